// esl_dense_objects.hip — esl_dense_objects (include/esl.h, "per-instance ellipsoids from the dense map"; the steps' numbers below are
// the header's; arithmetic and host decisions: esl_dense_obj.hpp).  It works on the dense map's sorted list (esl_dense_int.hpp, whose
// rule on stores and bounded probes holds here): k_dobj_gate (kept voxels, totals, the forest), k_dobj_union (connected components:
// esl_uf.hpp's lock-free union-find over neighbour probes of the voxel table), k_dobj_roots (real roots, size, samples), k_dobj_table
// (components of min_component voxels or more); the host sorts the table and picks a component per label (dobj_choose); k_dobj_rows /
// _box / _mom (integer moments of the chosen components), the host builds their frames, k_dobj_ext (extents), k_dobj_vout (every
// voxel's table row).
// Voxel i is the i-th entry of the sorted list: ascending packed key, so the smallest index of a set is its smallest key.  The forest
// `parent` is over these indices and links the larger root under the smaller one: a component's final root IS its key's voxel.
#include "esl_dense_int.hpp"
#include "esl_dense_obj.hpp"
#include "esl_uf.hpp"

namespace esl {

enum { DO_IN_RANGE, DO_GATED, DO_KEPT, DO_COMP_ALL, DO_ROWS, DO_COUNT };
// the call's buffers (DenseState::obj_set)
enum { DB_SIDX, DB_VLAB, DB_PARENT, DB_VROOT, DB_ROWOF, DB_CSIZE, DB_CSAMP, DB_OCTR, DB_LABKEPT, DB_TABLE, DB_ROWROOT, DB_ROWOBJ,
       DB_KBOX, DB_MOM, DB_AXES, DB_EXT, DB_VOUT, DB_OBJ_COUNT };
static_assert(DB_OBJ_COUNT == kDobjBufs, "esl_dense_int.hpp sizes DenseState::obj_set");

struct DobjArgs {
  const u64* keys; const DenseRec* rec; u64 H;
  const u64* skey; const unsigned int* sval; int n;
  int* sidx;                                   // H: table slot -> voxel index (written for the occupied slots only)
  int* vlab; int* parent; int* vroot; int* rowof;   // n: label of a kept voxel or -1; forest; root; table row of a ROOT (-2: none)
  unsigned int* csize; unsigned int* csamp;    // n: members and samples, at the root's index
  int N, min_votes, min_count, min_component, reach, n_off;
  double leaf, pn[3], pd, plane_dist;
  u64* ctr; int* labkept;                      // DO_*; N: kept voxels per label
  int* table; long long table_cap;
  const int* rowroot; const int* rowobj; int R;   // per sorted table row: its root, the object it is chosen for or -1
  int* kbox; u64* mom;                         // N x 6: kmin, kmax; N x kDobjMoments
  const double* axes; u64* ext;                // N x 9; N x 6: encoded minima, maxima
  int* vout; long long n_vout;
};

// Groups: the wave's active lanes (on) grouped by their value o -- a component's root or an object.  The list is in key order, so a
// wave sees few distinct values, but not in runs: two facing walls alternate voxel by voxel.  One round per distinct value, at most
// kDobjGroups rounds: the group's lanes are reduced by a butterfly in which the other lanes carry the neutral element, and lane 0
// emits the group's atomics; lanes left over after the rounds emit their own.  Measured on the synthetic room (435,218 members of
// eight components): k_dobj_mom 11.0 ms with one set of atomics per RUN of equal values, 0.43 ms with groups.
constexpr int kDobjGroups = 4;
struct DobjAdd { template <class T> __device__ __forceinline__ T operator()(T x, T y) const { return x + y; } };
struct DobjMin { template <class T> __device__ __forceinline__ T operator()(T x, T y) const { return y < x ? y : x; } };
struct DobjMax { template <class T> __device__ __forceinline__ T operator()(T x, T y) const { return y > x ? y : x; } };
template <int NV, class T, class Op, class Emit>
__device__ __forceinline__ void dobj_group_reduce(bool on, int o, const T (&v)[NV], T neutral, Op op, Emit emit) {
  const int lane = threadIdx.x & 63;
  u64 todo = __ballot(on);
  for (int round = 0; round < kDobjGroups && todo; ++round) {   // wave-uniform
    const int o0 = __shfl(o, __ffsll((long long)todo) - 1, 64);
    const bool mine = on && o == o0;
    T r[NV];
#pragma unroll
    for (int c = 0; c < NV; ++c) r[c] = mine ? v[c] : neutral;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
      for (int c = 0; c < NV; ++c) r[c] = op(r[c], __shfl_xor(r[c], off, 64));
    }
    if (lane == 0) emit(o0, r);
    todo &= ~__ballot(mine);
  }
  if ((todo >> lane) & 1) emit(o, v);
}

// step 1 over the sorted list: the three gates in order, the four totals by ballot + popcount, the forest and the per-voxel words
static __global__ __launch_bounds__(kDenseThreads) void k_dobj_gate(DobjArgs a) {
  const int lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * kDenseThreads + threadIdx.x;
  bool inr = false, gated = false, kept = false;
  if (i < a.n) {
    const unsigned int slot = a.sval[i];
    int label = -1;
    if (slot < a.H) {
      a.sidx[slot] = (int)i;
      const u64 best = a.rec[slot].best, count = a.rec[slot].count;
      if (best != 0) label = (int)~(unsigned)best;
      inr = label >= 0 && label < a.N;
      gated = inr && (best >> 32) >= (u64)a.min_votes && count >= (u64)a.min_count;
      if (gated) {
        int k[3];
        dense_unpack(a.skey[i], k);
        const double x[3] = {dobj_center(k[0], a.leaf), dobj_center(k[1], a.leaf), dobj_center(k[2], a.leaf)};
        kept = dobj_height(a.pn, a.pd, x) >= a.plane_dist;
      }
    }
    a.vlab[i] = kept ? label : -1;
    a.parent[i] = (int)i; a.vroot[i] = (int)i; a.rowof[i] = -2;
    a.csize[i] = 0; a.csamp[i] = 0;
  }
  const u64 m_r = __ballot(inr), m_g = __ballot(gated), m_k = __ballot(kept);
  if (lane == 0) {
    if (m_r) atomicAdd(&a.ctr[DO_IN_RANGE], (u64)__popcll(m_r));
    if (m_g) atomicAdd(&a.ctr[DO_GATED], (u64)__popcll(m_g));
    if (m_k) atomicAdd(&a.ctr[DO_KEPT], (u64)__popcll(m_k));
  }
}

// step 2.  Work item = (voxel i, one offset of the one-sided half of the (2 reach + 1)^3 - 1: those lexicographically above 0), offset
// major so that a wave takes consecutive voxels.  The neighbour's key is probed read-only in the voxel table (bounded by H); the
// union is esl_fit.hip's cl_union: cached walks, the linking CAS's return value is the truth and every retry continues from it.
static __global__ __launch_bounds__(kDenseThreads) void k_dobj_union(DobjArgs a) {
  const long long total = (long long)a.n * a.n_off, stride = (long long)gridDim.x * kDenseThreads;
  const int wd = 2 * a.reach + 1, first = (wd * wd * wd) / 2 + 1;
  for (long long w = (long long)blockIdx.x * kDenseThreads + threadIdx.x; w < total; w += stride) {
    const int o = (int)(w / a.n), i = (int)(w - (long long)o * a.n);
    const int lab = a.vlab[i];
    if (lab < 0) continue;
    int k[3];
    dense_unpack(a.skey[i], k);
    const int L = first + o;
    const int kx = k[0] + L / (wd * wd) - a.reach, ky = k[1] + (L / wd) % wd - a.reach, kz = k[2] + L % wd - a.reach;
    if (!dense_key_in_range(kx, ky, kz)) continue;
    const u64 key = dense_pack(kx, ky, kz);
    u64 slot = dense_hash(key) & (a.H - 1);
    int j = -1;
    for (u64 it = 0; it < a.H; ++it) {   // the table is read-only in this launch: cached loads
      const u64 cur = a.keys[slot];
      if (cur == key) {   // a dead slot (dense-map step 9) is no neighbour: it is not in the list and its sidx is stale
        if (a.rec[slot].count != 0) j = a.sidx[slot];
        break;
      }
      if (cur == kDenseEmpty) break;
      slot = (slot + 1) & (a.H - 1);
    }
    if (j < 0 || j >= a.n || a.vlab[j] != lab) continue;
    // equal parents, even stale ones, mean the two are joined already: components only ever merge
    if (__hip_atomic_load(&a.parent[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) ==
        __hip_atomic_load(&a.parent[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) continue;
    int ra = i, rb = j;
    for (;;) {
      ra = uf_find_cached(a.parent, ra); rb = uf_find_cached(a.parent, rb);
      if (ra == rb) break;
      if (ra < rb) { const int t = ra; ra = rb; rb = t; }
      const int seen = atomicCAS(&a.parent[ra], ra, rb);
      if (seen == ra) break;
      ra = seen;   // lost the race, or walked a stale copy of the forest: continue from ra's real parent
    }
  }
}

// the real roots (agent-scope loads), a launch after the unions; size and samples at the root, one pair of atomics per wave and root
static __global__ __launch_bounds__(kDenseThreads) void k_dobj_roots(DobjArgs a) {
  const long long i = (long long)blockIdx.x * kDenseThreads + threadIdx.x;
  const bool on = i < a.n && a.vlab[i] >= 0;
  int r = -1;
  unsigned int cnt = 0, smp = 0;
  if (on) {
    r = uf_find(a.parent, (int)i);
    a.vroot[i] = r;
    cnt = 1; smp = (unsigned int)a.rec[a.sval[i]].count;
  }
  const unsigned int v[2] = {cnt, smp};
  dobj_group_reduce(on, r, v, 0u, DobjAdd(), [&](int r0, const unsigned int (&t)[2]) {
    atomicAdd(&a.csize[r0], t[0]); atomicAdd(&a.csamp[r0], t[1]);
  });
}

// step 3 on the device: every root counts; those of min_component voxels or more take a row (in any order: the host sorts)
static __global__ __launch_bounds__(kDenseThreads) void k_dobj_table(DobjArgs a) {
  const long long i = (long long)blockIdx.x * kDenseThreads + threadIdx.x;
  const bool root = i < a.n && a.vlab[i] >= 0 && a.vroot[i] == (int)i;
  const u64 m = __ballot(root);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(&a.ctr[DO_COMP_ALL], (u64)__popcll(m));
  if (!root) return;
  const int lab = a.vlab[i];
  const unsigned int size = a.csize[i];
  atomicAdd(&a.labkept[lab], (int)size);
  if (size < (unsigned int)a.min_component) return;
  const long long row = (long long)atomicAdd(&a.ctr[DO_ROWS], 1ull);
  if (row >= a.table_cap) return;
  int k[3];
  dense_unpack(a.skey[i], k);
  int* t = a.table + row * kDobjRow;
  t[0] = lab; t[1] = (int)size; t[2] = (int)a.csamp[i]; t[3] = (int)i; t[4] = k[0]; t[5] = k[1]; t[6] = k[2]; t[7] = 0;
}

static __global__ __launch_bounds__(kDenseThreads) void k_dobj_rows(DobjArgs a) {
  const int r = blockIdx.x * kDenseThreads + threadIdx.x;
  if (r >= a.R) return;
  const int root = a.rowroot[r];
  if (root >= 0 && root < a.n) a.rowof[root] = r;
}

// the object whose chosen component voxel i belongs to, or -1
__device__ __forceinline__ int dobj_member(const DobjArgs& a, long long i) {
  if (i >= a.n || a.vlab[i] < 0) return -1;
  const int row = a.rowof[a.vroot[i]];
  if (row < 0 || row >= a.R) return -1;
  const int o = a.rowobj[row];
  return o < a.N ? o : -1;
}

// step 5, first pass: kmin and kmax of the chosen components
static __global__ __launch_bounds__(kDenseThreads) void k_dobj_box(DobjArgs a) {
  const long long i = (long long)blockIdx.x * kDenseThreads + threadIdx.x;
  const int o = dobj_member(a, i);
  const bool on = o >= 0;
  int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {INT_MIN, INT_MIN, INT_MIN};
  if (on) {
    dense_unpack(a.skey[i], lo);
    for (int c = 0; c < 3; ++c) hi[c] = lo[c];
  }
  dobj_group_reduce(on, o, lo, INT_MAX, DobjMin(), [&](int o0, const int (&t)[3]) {
    for (int c = 0; c < 3; ++c) atomicMin(&a.kbox[o0 * 6 + c], t[c]);
  });
  dobj_group_reduce(on, o, hi, INT_MIN, DobjMax(), [&](int o0, const int (&t)[3]) {
    for (int c = 0; c < 3; ++c) atomicMax(&a.kbox[o0 * 6 + 3 + c], t[c]);
  });
}

// step 5, second pass (a launch after the first): s and M relative to kmin, 64-bit integer sums
static __global__ __launch_bounds__(kDenseThreads) void k_dobj_mom(DobjArgs a) {
  const long long i = (long long)blockIdx.x * kDenseThreads + threadIdx.x;
  const int o = dobj_member(a, i);
  const bool on = o >= 0;
  u64 v[kDobjMoments];
  for (int c = 0; c < kDobjMoments; ++c) v[c] = 0;
  if (on) {
    int k[3];
    dense_unpack(a.skey[i], k);
    const long long d0 = (long long)k[0] - a.kbox[o * 6], d1 = (long long)k[1] - a.kbox[o * 6 + 1], d2 = (long long)k[2] - a.kbox[o * 6 + 2];
    v[0] = (u64)d0; v[1] = (u64)d1; v[2] = (u64)d2;
    v[3] = (u64)(d0 * d0); v[4] = (u64)(d0 * d1); v[5] = (u64)(d0 * d2); v[6] = (u64)(d1 * d1); v[7] = (u64)(d1 * d2); v[8] = (u64)(d2 * d2);
  }
  dobj_group_reduce(on, o, v, 0ull, DobjAdd(), [&](int o0, const u64 (&t)[kDobjMoments]) {
    for (int c = 0; c < kDobjMoments; ++c) atomicAdd(&a.mom[(size_t)o0 * kDobjMoments + c], t[c]);
  });
}

// step 7: the three projections of every member's centre; minima and maxima as 64-bit integers of the order-preserving encoding
static __global__ __launch_bounds__(kDenseThreads) void k_dobj_ext(DobjArgs a) {
  const long long i = (long long)blockIdx.x * kDenseThreads + threadIdx.x;
  const int o = dobj_member(a, i);
  const bool on = o >= 0;
  u64 lo[3] = {~0ull, ~0ull, ~0ull}, hi[3] = {0, 0, 0};
  if (on) {
    int k[3];
    dense_unpack(a.skey[i], k);
    const double p[3] = {dobj_center(k[0], a.leaf), dobj_center(k[1], a.leaf), dobj_center(k[2], a.leaf)};
    for (int c = 0; c < 3; ++c) lo[c] = hi[c] = dobj_enc(dobj_proj(a.axes + (size_t)o * 9 + 3 * c, p));
  }
  dobj_group_reduce(on, o, lo, ~0ull, DobjMin(), [&](int o0, const u64 (&t)[3]) {
    for (int c = 0; c < 3; ++c) atomicMin(&a.ext[(size_t)o0 * 6 + c], t[c]);
  });
  dobj_group_reduce(on, o, hi, 0ull, DobjMax(), [&](int o0, const u64 (&t)[3]) {
    for (int c = 0; c < 3; ++c) atomicMax(&a.ext[(size_t)o0 * 6 + 3 + c], t[c]);
  });
}

// step 9
static __global__ __launch_bounds__(kDenseThreads) void k_dobj_vout(DobjArgs a) {
  const long long i = (long long)blockIdx.x * kDenseThreads + threadIdx.x;
  if (i >= a.n_vout) return;
  a.vout[i] = a.vlab[i] < 0 ? -1 : a.rowof[a.vroot[i]];
}

}  // namespace esl

using namespace esl;

extern "C" void esl_dense_obj_params_default(esl_dense_obj_params* p) {
  if (!p) return;
  p->reach = 2; p->min_votes = 1; p->min_count = 1; p->min_component = 100; p->max_components = 65536; p->pad = 0; p->plane_dist = 0.05;
}

extern "C" int esl_dense_objects(esl_ctx* c, int32_t N, const double ground_world[4], const esl_dense_obj_params* pp, double* objs_out,
                                 int32_t* stats_out, int64_t comp_cap, int32_t* comp_out, int64_t voxel_cap, int32_t* voxel_comp_out,
                                 esl_dense_obj_result* out) {
  const char* who = "esl_dense_objects";
  if (!c) return dense_fail(ESL_ERR_INVALID, who, "null ctx");
  if (!ground_world) return dense_fail(ESL_ERR_INVALID, who, "null ground_world");
  if (!out) return dense_fail(ESL_ERR_INVALID, who, "null out");
  if (N < 0) return dense_fail(ESL_ERR_INVALID, who, "negative N");
  if (comp_cap < 0) return dense_fail(ESL_ERR_INVALID, who, "negative comp_cap");
  if (voxel_cap < 0) return dense_fail(ESL_ERR_INVALID, who, "negative voxel_cap");
  if (N > 0 && !objs_out) return dense_fail(ESL_ERR_INVALID, who, "null objs_out");
  if (comp_cap > 0 && !comp_out) return dense_fail(ESL_ERR_INVALID, who, "null comp_out with comp_cap > 0");
  if (voxel_cap > 0 && !voxel_comp_out) return dense_fail(ESL_ERR_INVALID, who, "null voxel_comp_out with voxel_cap > 0");
  DobjPlane pl;
  if (!dobj_plane(ground_world, pl)) return dense_fail(ESL_ERR_INVALID, who, "ground_world not finite or its normal shorter than 1e-12");
  esl_dense_obj_params p;
  if (pp) p = *pp; else esl_dense_obj_params_default(&p);
  if (p.reach < 1 || p.reach > 3) return dense_fail(ESL_ERR_INVALID, who, "reach outside 1 .. 3");
  if (p.min_votes < 1) return dense_fail(ESL_ERR_INVALID, who, "min_votes < 1");
  if (p.min_count < 1) return dense_fail(ESL_ERR_INVALID, who, "min_count < 1");
  if (p.min_component < 1) return dense_fail(ESL_ERR_INVALID, who, "min_component < 1");
  if (p.max_components < 1 || p.max_components > (1 << 20)) return dense_fail(ESL_ERR_INVALID, who, "max_components outside 1 .. 2^20");
  if (!std::isfinite(p.plane_dist)) return dense_fail(ESL_ERR_INVALID, who, "plane_dist not finite");
  if (!dense_begun(c, who)) return ESL_ERR_STATE;
  DenseState& d = *c->dense;
  if (!d.with_inst) return dense_fail(ESL_ERR_STATE, who, "the map was begun without labels");
  std::memset(out, 0, sizeof(*out));
  if (dense_map_invalid(d, out)) return ESL_OK;   // nothing is written
  const long long n = d.n_voxels;
  const long long n_comp_w_max = comp_cap, n_vox_w = std::min<long long>(n, voxel_cap);
  out->n_voxels = (int32_t)n;
  // what holds when nothing is kept: every object has status 1, no voxel is kept
  for (int64_t i = 0; i < (int64_t)N * 10; ++i) objs_out[i] = 0;
  if (stats_out) {
    for (int o = 0; o < N; ++o) { int32_t* st = stats_out + 6 * o; st[0] = 1; st[1] = 0; st[2] = 0; st[3] = -1; st[4] = 0; st[5] = 0; }
  }
  for (long long i = 0; i < n_vox_w; ++i) voxel_comp_out[i] = -1;
  if (n == 0) return ESL_OK;

  ESL_HIP_TRY(hipSetDevice(c->device));
  ScratchSet<DB_OBJ_COUNT>& s = d.obj_set;
  DenseList L;
  if (const int rc = dense_list_begin(c, d, L)) return rc;
  const DenseOutArgs& k = L.k;
  const long long table_cap = std::min<long long>(p.max_components, n);
  {
    const size_t sn = (size_t)n, sN = (size_t)N, st = (size_t)table_cap;
    const DenseSlot want[] = {
        {DB_SIDX, (size_t)d.H * 4}, {DB_VLAB, sn * 4}, {DB_PARENT, sn * 4}, {DB_VROOT, sn * 4}, {DB_ROWOF, sn * 4}, {DB_CSIZE, sn * 4},
        {DB_CSAMP, sn * 4}, {DB_OCTR, DO_COUNT * sizeof(u64)}, {DB_LABKEPT, sN * 4}, {DB_TABLE, st * kDobjRow * 4}, {DB_ROWROOT, st * 4},
        {DB_ROWOBJ, st * 4}, {DB_KBOX, sN * 6 * 4}, {DB_MOM, sN * kDobjMoments * 8}, {DB_AXES, sN * 9 * 8}, {DB_EXT, sN * 6 * 8},
        {DB_VOUT, (size_t)n_vox_w * 4}};
    if (const int rc = dense_grow(c, s, want, false)) return rc;
  }
  DobjArgs a;
  std::memset(&a, 0, sizeof(a));
  a.keys = k.keys; a.rec = k.rec; a.H = k.H; a.skey = k.skey; a.sval = k.sval; a.n = (int)n;
  a.sidx = s.at<int>(DB_SIDX); a.vlab = s.at<int>(DB_VLAB); a.parent = s.at<int>(DB_PARENT); a.vroot = s.at<int>(DB_VROOT);
  a.rowof = s.at<int>(DB_ROWOF); a.csize = s.at<unsigned int>(DB_CSIZE); a.csamp = s.at<unsigned int>(DB_CSAMP);
  a.N = N; a.min_votes = p.min_votes; a.min_count = p.min_count; a.min_component = p.min_component; a.reach = p.reach;
  a.n_off = ((2 * p.reach + 1) * (2 * p.reach + 1) * (2 * p.reach + 1) - 1) / 2;
  a.leaf = d.p.leaf; a.pd = pl.d; a.plane_dist = p.plane_dist;
  for (int i = 0; i < 3; ++i) a.pn[i] = pl.n[i];
  a.ctr = s.at<u64>(DB_OCTR); a.labkept = s.at<int>(DB_LABKEPT);
  a.table = s.at<int>(DB_TABLE); a.table_cap = table_cap;
  a.rowroot = s.at<int>(DB_ROWROOT); a.rowobj = s.at<int>(DB_ROWOBJ);
  a.kbox = s.at<int>(DB_KBOX); a.mom = s.at<u64>(DB_MOM); a.axes = s.at<double>(DB_AXES); a.ext = s.at<u64>(DB_EXT);
  a.vout = s.at<int>(DB_VOUT); a.n_vout = n_vox_w;
  const dim3 blk(kDenseThreads), grid_n(dense_blocks((u64)n));

  // steps 1 to 3 on the device
  ESL_HIP_TRY(hipMemsetAsync(a.ctr, 0, DO_COUNT * sizeof(u64), c->stream));
  if (N > 0) ESL_HIP_TRY(hipMemsetAsync(a.labkept, 0, (size_t)N * 4, c->stream));
  {
    ProfScope ps(c, 4);
    if (const int rc = dense_list_launch(c, d, L, true, false)) return rc;
    hipLaunchKernelGGL(k_dobj_gate, grid_n, blk, 0, c->stream, a);
    const u64 items = (u64)n * (u64)a.n_off;
    hipLaunchKernelGGL(k_dobj_union, dim3(std::min<unsigned>(dense_blocks(std::min<u64>(items, 1ull << 40)), 1u << 16)), blk, 0, c->stream, a);
    hipLaunchKernelGGL(k_dobj_roots, grid_n, blk, 0, c->stream, a);
    hipLaunchKernelGGL(k_dobj_table, grid_n, blk, 0, c->stream, a);
  }
  ESL_HIP_TRY(hipGetLastError());
  u64 ctr[DO_COUNT];
  ESL_HIP_TRY(hipMemcpyAsync(ctr, a.ctr, sizeof(ctr), hipMemcpyDeviceToHost, c->stream));
  ESL_HIP_TRY(hipStreamSynchronize(c->stream));
  out->n_in_range = (int32_t)ctr[DO_IN_RANGE]; out->n_gated = (int32_t)ctr[DO_GATED]; out->n_kept = (int32_t)ctr[DO_KEPT];
  out->n_components_all = (int32_t)ctr[DO_COMP_ALL]; out->n_components = (int32_t)ctr[DO_ROWS];
  const long long R = (long long)ctr[DO_ROWS];
  if (R > p.max_components) {   // step 3: a result; the object, table and voxel outputs are zero / -1
    out->status = 3;
    if (stats_out) std::memset(stats_out, 0, (size_t)N * 6 * sizeof(int32_t));
    const long long cw = std::min<long long>(R, n_comp_w_max);
    if (cw > 0) std::memset(comp_out, 0, (size_t)cw * 6 * sizeof(int32_t));
    return ESL_OK;
  }

  // the table on the host: sorted (step 3), the chosen row per label (step 4)
  std::vector<int> tab((size_t)R * kDobjRow), labkept((size_t)N);
  if (R > 0) ESL_HIP_TRY(hipMemcpyAsync(tab.data(), a.table, tab.size() * 4, hipMemcpyDeviceToHost, c->stream));
  if (N > 0) ESL_HIP_TRY(hipMemcpyAsync(labkept.data(), a.labkept, (size_t)N * 4, hipMemcpyDeviceToHost, c->stream));
  ESL_HIP_TRY(hipStreamSynchronize(c->stream));
  DobjChoice ch;
  dobj_choose(tab.data(), R, N, n_comp_w_max, comp_out, ch);
  std::vector<int> kbox((size_t)N * 6);
  for (int o = 0; o < N; ++o) for (int e = 0; e < 6; ++e) kbox[(size_t)o * 6 + e] = e < 3 ? INT_MAX : INT_MIN;
  if (R > 0) {
    ESL_HIP_TRY(hipMemcpyAsync(s.buf[DB_ROWROOT], ch.rowroot.data(), (size_t)R * 4, hipMemcpyHostToDevice, c->stream));
    ESL_HIP_TRY(hipMemcpyAsync(s.buf[DB_ROWOBJ], ch.rowobj.data(), (size_t)R * 4, hipMemcpyHostToDevice, c->stream));
  }
  if (N > 0) {
    ESL_HIP_TRY(hipMemcpyAsync(a.kbox, kbox.data(), kbox.size() * 4, hipMemcpyHostToDevice, c->stream));
    ESL_HIP_TRY(hipMemsetAsync(a.mom, 0, (size_t)N * kDobjMoments * 8, c->stream));
  }
  a.R = (int)R;
  const bool any_chosen = R > 0 && N > 0;
  {
    ProfScope ps(c, 4);
    if (R > 0) hipLaunchKernelGGL(k_dobj_rows, dim3(dense_blocks((u64)R)), blk, 0, c->stream, a);
    if (any_chosen) {
      hipLaunchKernelGGL(k_dobj_box, grid_n, blk, 0, c->stream, a);
      hipLaunchKernelGGL(k_dobj_mom, grid_n, blk, 0, c->stream, a);
    }
  }
  ESL_HIP_TRY(hipGetLastError());
  std::vector<long long> mom((size_t)N * kDobjMoments);
  if (any_chosen) {
    ESL_HIP_TRY(hipMemcpyAsync(kbox.data(), a.kbox, kbox.size() * 4, hipMemcpyDeviceToHost, c->stream));
    ESL_HIP_TRY(hipMemcpyAsync(mom.data(), a.mom, mom.size() * 8, hipMemcpyDeviceToHost, c->stream));
  }
  ESL_HIP_TRY(hipStreamSynchronize(c->stream));

  // steps 4 to 6 on the host: statuses, the guard, the frames
  std::vector<int> status((size_t)N, 0);
  std::vector<double> axes((size_t)N * 9, 0.0);
  std::vector<u64> ext((size_t)N * 6);
  for (int o = 0; o < N; ++o) {
    for (int e = 0; e < 6; ++e) ext[(size_t)o * 6 + e] = e < 3 ? ~0ull : 0ull;
    const int row = ch.chosen[(size_t)o];
    const long long size = row >= 0 ? tab[(size_t)ch.order[(size_t)row] * kDobjRow + 1] : 0;
    status[(size_t)o] = dobj_status(labkept[(size_t)o], row, kbox.data() + (size_t)o * 6, size);
    if (status[(size_t)o] == 0) dobj_frame(pl, size, mom.data() + (size_t)o * kDobjMoments, axes.data() + (size_t)o * 9);
  }
  if (N > 0) {
    ESL_HIP_TRY(hipMemcpyAsync(s.buf[DB_AXES], axes.data(), axes.size() * 8, hipMemcpyHostToDevice, c->stream));
    ESL_HIP_TRY(hipMemcpyAsync(a.ext, ext.data(), ext.size() * 8, hipMemcpyHostToDevice, c->stream));
  }
  {
    ProfScope ps(c, 4);
    if (any_chosen) hipLaunchKernelGGL(k_dobj_ext, grid_n, blk, 0, c->stream, a);
    if (n_vox_w > 0) hipLaunchKernelGGL(k_dobj_vout, dim3(dense_blocks((u64)n_vox_w)), blk, 0, c->stream, a);
  }
  ESL_HIP_TRY(hipGetLastError());
  if (any_chosen) ESL_HIP_TRY(hipMemcpyAsync(ext.data(), a.ext, ext.size() * 8, hipMemcpyDeviceToHost, c->stream));
  if (n_vox_w > 0) ESL_HIP_TRY(hipMemcpyAsync(voxel_comp_out, a.vout, (size_t)n_vox_w * 4, hipMemcpyDeviceToHost, c->stream));
  ESL_HIP_TRY(hipStreamSynchronize(c->stream));

  // steps 7 and 8
  for (int o = 0; o < N; ++o) {
    const int st = status[(size_t)o], row = ch.chosen[(size_t)o];
    if (st == 0) {
      double mn[3], mx[3];
      for (int e = 0; e < 3; ++e) { mn[e] = dobj_dec(ext[(size_t)o * 6 + e]); mx[e] = dobj_dec(ext[(size_t)o * 6 + 3 + e]); }
      dobj_row(axes.data() + (size_t)o * 9, mn, mx, d.p.leaf, objs_out + (size_t)o * 10);
      ++out->n_ok;
    }
    if (stats_out) {
      int32_t* so = stats_out + 6 * o;
      const int* t = row >= 0 ? tab.data() + (size_t)ch.order[(size_t)row] * kDobjRow : nullptr;
      so[0] = st; so[1] = labkept[(size_t)o]; so[2] = ch.nrows[(size_t)o]; so[3] = row; so[4] = t ? t[1] : 0; so[5] = t ? t[2] : 0;
    }
  }
  return ESL_OK;
}
