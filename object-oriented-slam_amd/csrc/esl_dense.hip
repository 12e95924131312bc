// esl_dense.hip — esl_dense_*: the voxel-fused dense map of many RGB-D frames (include/esl.h, "the dense map"; the steps' numbers
// below are the header's).  The per-sample arithmetic is esl_dense_key.hpp's; this file holds the tables and the kernels.
//   the voxel table   H = the smallest power of two >= 2 max_voxels slots: a packed key per slot (all ones = empty) and one 64-byte
//                     record {S_x, S_y, S_z, sum B, sum G, sum R, count, best}, every field a 64-bit integer.
//   the pair table    2 H slots: key = voxel slot << 32 | id (all ones = empty), a 32-bit count.
//   k_dense_insert    one lane per sampled pixel, consecutive lanes on consecutive sampled columns (the flat sample index of a frame
//                     wraps from one sampled row to the next).  A workgroup's frame is uniform, so its R, t and K are scalar loads.
//                     Steps 1-3 per lane; the five counts by ballot + popcount, one atomic per wave and count.  The lane's voxel slot
//                     is found by hash64 + linear probing with a 64-bit atomicCAS, bounded by H; the sums are 64-bit integer atomics,
//                     the vote one more probe in the pair table.
//                     COMBINE: lanes of a wave whose key equals their left neighbour's form a run; the run's integer sums are folded
//                     into its first lane by a segmented shuffle scan and only run heads touch the voxel table; the run's lanes then
//                     learn the head's slot and fold their votes per (run, id) the same way.  Integer sums: both forms give the same
//                     bits.  ESL_DENSE_COMBINE=0 / 1 picks the form (read by esl_dense_begin; measurement: scripts/dense_map_bench.py).
//   k_dense_compact   extract: the occupied slots as (packed key, slot), appended with one atomic per wave; clears the best words
//   k_dense_vote      extract: per occupied pair one atomicMax of (votes << 32 | ~id) into its voxel's best word: most votes, ties to
//                     the lowest id.  Done at extract time over the whole pair table, so incremental adds stay exact.
//   rocprim radix sort of (packed key, slot), then k_dense_gather writes the first `cap` voxels in key order.
// Every store to global memory is a vector store or an atomic in plain C++; no loop waits for another thread: a probe that finds no
// slot within the table's size, or a map over its capacity, raises the sticky status 3 and gives up.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "esl_ctx.hpp"
#include "esl_dense_key.hpp"

namespace esl {

static_assert(sizeof(esl_dense_params) == 40, "include/esl.h states this size");
static_assert(sizeof(esl_dense_add_result) == 48, "include/esl.h states this size");
static_assert(sizeof(esl_dense_info) == 32, "include/esl.h states this size");

constexpr int kDenseThreads = 256;
constexpr int kDenseMaxVoxels = 1 << 26;
typedef unsigned long long u64;

struct DenseRec { long long S[3]; u64 col[3]; u64 count; u64 best; };
static_assert(sizeof(DenseRec) == 64, "one record per 64-byte segment");

// the device counters: this call's five counts, then what lives as long as the map
enum { DC_SAMPLED, DC_ZERO, DC_DEPTH_OUT, DC_KEY_OUT, DC_USED, DC_VOXELS, DC_PAIRS, DC_STATUS, DC_LIST, DC_COUNT };

struct DenseArgs {
  const double* pose; int F;
  double K[4];
  int rows, cols, stride, srows, scols;
  const unsigned short* depth; const unsigned char* bgr; const int* inst;   // bgr / inst null: not kept
  double leaf, depth_scale, depth_min, depth_max;
  u64* keys; DenseRec* rec; u64* pkeys; unsigned int* pcnt;
  u64 H, P, max_voxels, max_pairs;
  u64* ctr;
};

enum { DB_KEYS, DB_REC, DB_PKEYS, DB_PCNT, DB_CTR, DB_POSE, DB_DEPTH, DB_BGR, DB_INST, DB_LKEY, DB_LVAL, DB_SKEY, DB_SVAL, DB_TEMP,
       DB_OKEY, DB_OXYZ, DB_OCNT, DB_OBGR, DB_OINST, DB_OVOTES, DB_COUNT };
struct DenseState {
  ScratchSet<DB_COUNT> set;
  bool begun = false, combine = true;
  esl_dense_params p;
  int with_color = 0, with_inst = 0;
  u64 H = 0;
  long long n_samples = 0, n_voxels = 0, n_pairs = 0;
  int status = 0;
  std::vector<double> cams, pose;   // host staging of a call's poses
};

__device__ __forceinline__ u64 dense_hash(u64 k) {   // hash64 of esl_fit.hip
  k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
  return k;
}
__device__ __forceinline__ void dense_overflow(u64* ctr) { atomicMax(&ctr[DC_STATUS], 3ull); }
__device__ __forceinline__ bool dense_over(const u64* ctr) {
  return __hip_atomic_load(&ctr[DC_STATUS], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
}

// The slot of `key` in a table of n (a power of two) slots, claimed if new; -1 when the map is over its capacity.  A new key counts
// in ctr[which] and raises status 3 beyond `limit`.  At most n probes; every 32nd one looks at the status, so that a table filling up
// ends the call's remaining probes early.
__device__ __forceinline__ long long dense_find(u64* keys, u64 n, u64 key, u64* ctr, int which, u64 limit) {
  u64 slot = dense_hash(key) & (n - 1);
  for (u64 it = 0; it < n; ++it) {
    u64 cur = __hip_atomic_load(&keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == kDenseEmpty) {
      cur = atomicCAS(&keys[slot], kDenseEmpty, key);
      if (cur == kDenseEmpty) {
        if (atomicAdd(&ctr[which], 1ull) >= limit) dense_overflow(ctr);
        return (long long)slot;
      }
    }
    if (cur == key) return (long long)slot;
    if ((it & 31) == 31 && dense_over(ctr)) return -1;
    slot = (slot + 1) & (n - 1);
  }
  dense_overflow(ctr);
  return -1;
}

// segmented sum towards the first lane of every run: rid = the run's number (non-decreasing along the wave)
template <class T>
__device__ __forceinline__ T dense_run_sum(T v, int rid, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const T o = __shfl_down(v, off, 64);
    const int orid = __shfl_down(rid, off, 64);
    if (lane + off < 64 && orid == rid) v += o;
  }
  return v;
}

// grid = (blocks over the sampled pixels of a frame, frames: at most 65535, a workgroup takes blockIdx.y, + gridDim.y, ...)
template <bool COMBINE>
static __global__ __launch_bounds__(kDenseThreads) void k_dense_insert(DenseArgs a) {
  const int lane = threadIdx.x & 63;
  const u64 le = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);   // the lanes up to and including this one
  const long long per = (long long)a.srows * a.scols;
  const long long i = (long long)blockIdx.x * kDenseThreads + threadIdx.x;
  const bool in = i < per;
  int row = 0, col = 0;
  if (in) {
    const int sr = (int)(i / a.scols);
    row = sr * a.stride; col = (int)(i - (long long)sr * a.scols) * a.stride;   // row < rows, col < cols
  }
  for (int f = blockIdx.y; f < a.F; f += gridDim.y) {
    const double* P = a.pose + (size_t)f * kDensePose;
    int cat = -1, id = -1;
    u64 key = kDenseEmpty, rgbc = 0;   // sum B | sum G << 16 | sum R << 32 | count << 48: a wave's sums stay below 2^16
    long long s0 = 0, s1 = 0, s2 = 0;
    if (in) {
      const size_t px = ((size_t)f * a.rows + row) * a.cols + col;
      double pc[3], pw[3];
      int k[3];
      cat = dense_sample(a.depth[px], col, row, a.K, a.depth_scale, a.depth_min, a.depth_max, pc);
      if (cat == DENSE_USED) {
        dense_world(P, pc, pw);
        if (dense_key(pw, a.leaf, k)) {
          key = dense_pack(k[0], k[1], k[2]);
          s0 = dense_fix(pw[0]); s1 = dense_fix(pw[1]); s2 = dense_fix(pw[2]);
          rgbc = 1ull << 48;
          if (a.bgr) rgbc |= (u64)a.bgr[px * 3] | (u64)a.bgr[px * 3 + 1] << 16 | (u64)a.bgr[px * 3 + 2] << 32;
          if (a.inst) id = a.inst[px];
        } else {
          cat = DENSE_KEY_OUT;
        }
      }
    }
    {   // the call's counts: one atomic per wave and count
      const u64 m_in = __ballot(in), m_z = __ballot(cat == DENSE_ZERO), m_d = __ballot(cat == DENSE_DEPTH_OUT),
                m_k = __ballot(cat == DENSE_KEY_OUT), m_u = __ballot(cat == DENSE_USED);
      if (lane == 0) {
        if (m_in) atomicAdd(&a.ctr[DC_SAMPLED], (u64)__popcll(m_in));
        if (m_z) atomicAdd(&a.ctr[DC_ZERO], (u64)__popcll(m_z));
        if (m_d) atomicAdd(&a.ctr[DC_DEPTH_OUT], (u64)__popcll(m_d));
        if (m_k) atomicAdd(&a.ctr[DC_KEY_OUT], (u64)__popcll(m_k));
        if (m_u) atomicAdd(&a.ctr[DC_USED], (u64)__popcll(m_u));
      }
    }
    const bool used = cat == DENSE_USED;
    long long slot = -1;
    if (!COMBINE) {
      if (used) {
        slot = dense_find(a.keys, a.H, key, a.ctr, DC_VOXELS, a.max_voxels);
        if (slot >= 0) {
          DenseRec* r = a.rec + slot;
          atomicAdd((u64*)&r->S[0], (u64)s0); atomicAdd((u64*)&r->S[1], (u64)s1); atomicAdd((u64*)&r->S[2], (u64)s2);
          atomicAdd(&r->count, 1ull);
          if (a.bgr) {
            atomicAdd(&r->col[0], rgbc & 0xFFFFull); atomicAdd(&r->col[1], (rgbc >> 16) & 0xFFFFull);
            atomicAdd(&r->col[2], (rgbc >> 32) & 0xFFFFull);
          }
          if (a.pkeys && id >= 0) {
            const long long ps = dense_find(a.pkeys, a.P, (u64)slot << 32 | (u64)(unsigned)id, a.ctr, DC_PAIRS, a.max_pairs);
            if (ps >= 0) atomicAdd(&a.pcnt[ps], 1u);
          }
        }
      }
    } else {
      // runs: a lane that is not used is a run of its own with nothing to add
      const u64 kprev = __shfl_up(key, 1, 64);
      const bool head = !used || lane == 0 || kprev != key;
      const u64 hm = __ballot(head);
      const int rid = __popcll(hm & le);
      s0 = dense_run_sum(s0, rid, lane); s1 = dense_run_sum(s1, rid, lane); s2 = dense_run_sum(s2, rid, lane);
      rgbc = dense_run_sum(rgbc, rid, lane);
      if (used && head) {
        slot = dense_find(a.keys, a.H, key, a.ctr, DC_VOXELS, a.max_voxels);
        if (slot >= 0) {
          DenseRec* r = a.rec + slot;
          atomicAdd((u64*)&r->S[0], (u64)s0); atomicAdd((u64*)&r->S[1], (u64)s1); atomicAdd((u64*)&r->S[2], (u64)s2);
          atomicAdd(&r->count, rgbc >> 48);
          if (a.bgr) {
            atomicAdd(&r->col[0], rgbc & 0xFFFFull); atomicAdd(&r->col[1], (rgbc >> 16) & 0xFFFFull);
            atomicAdd(&r->col[2], (rgbc >> 32) & 0xFFFFull);
          }
        }
      }
      if (a.pkeys) {   // workgroup-uniform
        const int hl = 63 - __clzll((long long)(hm & le));   // the head of this lane's run; lane 0 is always a head
        const long long rslot = __shfl(slot, hl, 64);
        const bool vused = used && id >= 0 && rslot >= 0;
        const u64 vkey = vused ? ((u64)rslot << 32 | (u64)(unsigned)id) : kDenseEmpty;
        const u64 vprev = __shfl_up(vkey, 1, 64);
        const bool vhead = !vused || lane == 0 || vprev != vkey;
        const int vrid = __popcll(__ballot(vhead) & le);
        const int votes = dense_run_sum(vused ? 1 : 0, vrid, lane);
        if (vused && vhead) {
          const long long ps = dense_find(a.pkeys, a.P, vkey, a.ctr, DC_PAIRS, a.max_pairs);
          if (ps >= 0) atomicAdd(&a.pcnt[ps], (unsigned)votes);
        }
      }
    }
  }
}

struct DenseOutArgs {
  const u64* keys; DenseRec* rec; const u64* pkeys; const unsigned int* pcnt;
  u64 H, P;
  u64* ctr;
  u64* lkey; unsigned int* lval; u64 list_cap;          // compact
  const u64* skey; const unsigned int* sval; long long n_write;   // gather
  int with_color;
  int* okey; double* oxyz; int* ocnt; unsigned char* obgr; int* oinst; int* ovotes;   // null: not asked for
};

static __global__ __launch_bounds__(kDenseThreads) void k_dense_compact(DenseOutArgs a) {
  const int lane = threadIdx.x & 63;
  const u64 i = (u64)blockIdx.x * kDenseThreads + threadIdx.x;
  u64 key = kDenseEmpty;
  if (i < a.H) key = a.keys[i];
  const bool occ = key != kDenseEmpty;
  if (occ) a.rec[i].best = 0;
  const u64 m = __ballot(occ);
  u64 base = 0;
  if (lane == 0 && m) base = atomicAdd(&a.ctr[DC_LIST], (u64)__popcll(m));
  base = __shfl(base, 0, 64);
  if (occ) {
    const u64 pos = base + (u64)__popcll(m & ((1ull << lane) - 1ull));
    if (pos < a.list_cap) { a.lkey[pos] = key; a.lval[pos] = (unsigned int)i; }
  }
}

static __global__ __launch_bounds__(kDenseThreads) void k_dense_vote(DenseOutArgs a) {
  const u64 i = (u64)blockIdx.x * kDenseThreads + threadIdx.x;
  if (i >= a.P) return;
  const u64 key = a.pkeys[i];
  if (key == kDenseEmpty) return;
  const u64 slot = key >> 32;
  if (slot < a.H) atomicMax(&a.rec[slot].best, (u64)a.pcnt[i] << 32 | (u64)(unsigned)~(unsigned)key);
}

static __global__ __launch_bounds__(kDenseThreads) void k_dense_gather(DenseOutArgs a) {
  const long long i = (long long)blockIdx.x * kDenseThreads + threadIdx.x;
  if (i >= a.n_write) return;
  const unsigned int slot = a.sval[i];
  if (slot >= a.H) return;
  const DenseRec r = a.rec[slot];
  if (a.okey) {
    int k[3];
    dense_unpack(a.skey[i], k);
    a.okey[i * 3] = k[0]; a.okey[i * 3 + 1] = k[1]; a.okey[i * 3 + 2] = k[2];
  }
  if (a.oxyz) {
    for (int c = 0; c < 3; ++c) a.oxyz[i * 3 + c] = dense_mean(r.S[c], (long long)r.count);
  }
  if (a.ocnt) a.ocnt[i] = (int)r.count;
  if (a.obgr) {
    for (int c = 0; c < 3; ++c) a.obgr[i * 3 + c] = a.with_color ? (unsigned char)dense_color(r.col[c], r.count) : (unsigned char)0;
  }
  const bool voted = r.best != 0;
  if (a.oinst) a.oinst[i] = voted ? (int)~(unsigned)r.best : -1;
  if (a.ovotes) a.ovotes[i] = voted ? (int)(r.best >> 32) : 0;
}

void dense_scratch_stats(const esl_ctx* c, int64_t* allocs, int64_t* bytes) {
  if (c->dense) { *allocs = c->dense->set.allocs(); *bytes = (int64_t)c->dense->set.held(); }
}

void dense_release(esl_ctx* c) {   // called by esl_ctx_destroy
  if (c->dense) c->dense->set.release();
  delete c->dense;
  c->dense = nullptr;
}

}  // namespace esl

using namespace esl;

namespace {

int dense_fail(int rc, const char* who, const char* what) {
  set_error(std::string(who) + ": " + what);
  return rc;
}

unsigned dense_blocks(u64 n) { return (unsigned)((n + kDenseThreads - 1) / kDenseThreads); }

}  // namespace

extern "C" void esl_dense_params_default(esl_dense_params* p) {
  if (!p) return;
  p->leaf = 0.01; p->depth_scale = 5000.0; p->depth_min = 0.5; p->depth_max = 6.0; p->stride = 1; p->max_voxels = 1048576;
}

extern "C" int esl_debug_dense_allocs(esl_ctx* c, int64_t* allocs_out, int64_t* bytes_out) {
  if (!c || !allocs_out || !bytes_out) return dense_fail(ESL_ERR_INVALID, "esl_debug_dense_allocs", "null pointer");
  *allocs_out = 0; *bytes_out = 0;
  dense_scratch_stats(c, allocs_out, bytes_out);
  return ESL_OK;
}

extern "C" int esl_dense_begin(esl_ctx* c, const esl_dense_params* pp, int32_t with_color, int32_t with_inst) {
  const char* who = "esl_dense_begin";
  if (!c) return dense_fail(ESL_ERR_INVALID, who, "null ctx");
  esl_dense_params p;
  if (pp) p = *pp; else esl_dense_params_default(&p);
  if (!std::isfinite(p.leaf) || !(p.leaf > 0)) return dense_fail(ESL_ERR_INVALID, who, "leaf not finite or <= 0");
  if (!std::isfinite(p.depth_scale) || !(p.depth_scale > 0)) return dense_fail(ESL_ERR_INVALID, who, "depth_scale not finite or <= 0");
  if (!std::isfinite(p.depth_min)) return dense_fail(ESL_ERR_INVALID, who, "depth_min not finite");
  if (!std::isfinite(p.depth_max)) return dense_fail(ESL_ERR_INVALID, who, "depth_max not finite");
  if (p.depth_min > p.depth_max) return dense_fail(ESL_ERR_INVALID, who, "depth_min > depth_max");
  if (p.stride < 1) return dense_fail(ESL_ERR_INVALID, who, "stride < 1");
  if (p.max_voxels < 1 || p.max_voxels > kDenseMaxVoxels) return dense_fail(ESL_ERR_INVALID, who, "max_voxels outside 1 .. 2^26");
  if (with_color < 0 || with_inst < 0) return dense_fail(ESL_ERR_INVALID, who, "negative with_color or with_inst");
  ESL_HIP_TRY(hipSetDevice(c->device));
  if (!c->dense) c->dense = new DenseState();
  DenseState& d = *c->dense;
  d.begun = false;
  u64 H = 2;
  while (H < 2ull * (u64)p.max_voxels) H <<= 1;
  ScratchSet<DB_COUNT>& s = d.set;
  if (const int rc = s.grow(c, DB_KEYS, H * sizeof(u64))) return rc;
  if (const int rc = s.grow(c, DB_REC, H * sizeof(DenseRec))) return rc;
  if (const int rc = s.grow(c, DB_CTR, DC_COUNT * sizeof(u64))) return rc;
  ESL_HIP_TRY(hipMemsetAsync(s.buf[DB_KEYS], 0xFF, H * sizeof(u64), c->stream));
  ESL_HIP_TRY(hipMemsetAsync(s.buf[DB_REC], 0, H * sizeof(DenseRec), c->stream));
  ESL_HIP_TRY(hipMemsetAsync(s.buf[DB_CTR], 0, DC_COUNT * sizeof(u64), c->stream));
  if (with_inst) {
    if (const int rc = s.grow(c, DB_PKEYS, 2 * H * sizeof(u64))) return rc;
    if (const int rc = s.grow(c, DB_PCNT, 2 * H * sizeof(unsigned int))) return rc;
    ESL_HIP_TRY(hipMemsetAsync(s.buf[DB_PKEYS], 0xFF, 2 * H * sizeof(u64), c->stream));
    ESL_HIP_TRY(hipMemsetAsync(s.buf[DB_PCNT], 0, 2 * H * sizeof(unsigned int), c->stream));
  }
  ESL_HIP_TRY(hipStreamSynchronize(c->stream));
  const char* ev = std::getenv("ESL_DENSE_COMBINE");
  d.combine = !(ev && ev[0] == '0');
  d.p = p; d.with_color = with_color != 0; d.with_inst = with_inst != 0; d.H = H;
  d.n_samples = 0; d.n_voxels = 0; d.n_pairs = 0; d.status = 0;
  d.begun = true;
  return ESL_OK;
}

extern "C" int esl_dense_end(esl_ctx* c) {
  if (!c) return dense_fail(ESL_ERR_INVALID, "esl_dense_end", "null ctx");
  if (c->dense) c->dense->begun = false;
  return ESL_OK;
}

extern "C" int esl_dense_info_get(esl_ctx* c, esl_dense_info* out) {
  const char* who = "esl_dense_info_get";
  if (!c || !out) return dense_fail(ESL_ERR_INVALID, who, "null pointer");
  if (!c->dense || !c->dense->begun) return dense_fail(ESL_ERR_STATE, who, "no esl_dense_begin before");
  const DenseState& d = *c->dense;
  out->n_samples = d.n_samples;
  out->n_voxels = d.status ? -1 : (int32_t)d.n_voxels;
  out->n_pairs = d.status ? -1 : (int32_t)d.n_pairs;
  out->status = d.status; out->with_color = d.with_color; out->with_inst = d.with_inst; out->pad = 0;
  return ESL_OK;
}

extern "C" int esl_dense_add_frames(esl_ctx* c, const double* cams, int32_t F, const double K[4], int32_t rows, int32_t cols,
                                    const uint16_t* depth, const uint8_t* bgr, const int32_t* inst, esl_dense_add_result* out) {
  const char* who = "esl_dense_add_frames";
  if (!c) return dense_fail(ESL_ERR_INVALID, who, "null ctx");
  if (F < 0) return dense_fail(ESL_ERR_INVALID, who, "negative F");
  if (!K) return dense_fail(ESL_ERR_INVALID, who, "null K");
  if (rows < 1 || rows > kDenseMaxDim) return dense_fail(ESL_ERR_INVALID, who, "rows < 1 or > 16384");
  if (cols < 1 || cols > kDenseMaxDim) return dense_fail(ESL_ERR_INVALID, who, "cols < 1 or > 16384");
  if (!std::isfinite(K[0]) || !(K[0] > 0)) return dense_fail(ESL_ERR_INVALID, who, "fx not finite or <= 0");
  if (!std::isfinite(K[1]) || !(K[1] > 0)) return dense_fail(ESL_ERR_INVALID, who, "fy not finite or <= 0");
  if (F > 0 && !depth) return dense_fail(ESL_ERR_INVALID, who, "null depth");
  if (!c->dense || !c->dense->begun) return dense_fail(ESL_ERR_STATE, who, "no esl_dense_begin before");
  DenseState& d = *c->dense;
  if (F > 0 && d.with_color && !bgr) return dense_fail(ESL_ERR_STATE, who, "null bgr on a map begun with colour");
  if (F > 0 && d.with_inst && !inst) return dense_fail(ESL_ERR_STATE, who, "null inst on a map begun with labels");
  if (const int rc = resident_source_check(c, who, !cams && F > 0, F, false, 0)) return rc;
  if (out) { std::memset(out, 0, sizeof(*out)); out->status = d.status; }
  if (F == 0 || d.status) return ESL_OK;   // nothing to add; or over capacity: nothing more is added until the next esl_dense_begin
  ESL_HIP_TRY(hipSetDevice(c->device));
  // the poses: R and t of every frame on the host, before anything is added
  d.cams.resize((size_t)F * 7);
  if (cams) std::memcpy(d.cams.data(), cams, (size_t)F * 7 * sizeof(double));
  else {
    ESL_HIP_TRY(hipMemcpyAsync(d.cams.data(), c->cams, (size_t)F * 7 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    ESL_HIP_TRY(hipStreamSynchronize(c->stream));
  }
  d.pose.resize((size_t)F * kDensePose);
  for (int f = 0; f < F; ++f) {
    if (!dense_pose(d.cams.data() + (size_t)f * 7, d.pose.data() + (size_t)f * kDensePose))
      return dense_fail(ESL_ERR_INVALID, who, "a pose with a non-finite number or a quaternion of norm 0");
  }
  const int srows = (rows + d.p.stride - 1) / d.p.stride, scols = (cols + d.p.stride - 1) / d.p.stride;
  const long long per = (long long)srows * scols;
  if (d.n_samples + per * F >= (1ll << 31)) return dense_fail(ESL_ERR_INVALID, who, "n_samples would reach 2^31");
  ScratchSet<DB_COUNT>& s = d.set;
  const size_t n_img = (size_t)F * rows * cols;
  DenseArgs k;
  std::memset(&k, 0, sizeof(k));
  if (const int rc = upload(c, s, DB_POSE, (const double*)d.pose.data(), (size_t)F * kDensePose * sizeof(double), &k.pose)) return rc;
  if (const int rc = upload(c, s, DB_DEPTH, depth, n_img * sizeof(uint16_t), &k.depth)) return rc;
  if (d.with_color) { if (const int rc = upload(c, s, DB_BGR, bgr, n_img * 3, &k.bgr)) return rc; }
  if (d.with_inst) { if (const int rc = upload(c, s, DB_INST, inst, n_img * sizeof(int32_t), &k.inst)) return rc; }
  k.F = F; k.rows = rows; k.cols = cols; k.stride = d.p.stride; k.srows = srows; k.scols = scols;
  for (int i = 0; i < 4; ++i) k.K[i] = K[i];
  k.leaf = d.p.leaf; k.depth_scale = d.p.depth_scale; k.depth_min = d.p.depth_min; k.depth_max = d.p.depth_max;
  k.keys = s.at<u64>(DB_KEYS); k.rec = s.at<DenseRec>(DB_REC);
  if (d.with_inst) { k.pkeys = s.at<u64>(DB_PKEYS); k.pcnt = s.at<unsigned int>(DB_PCNT); }
  k.H = d.H; k.P = 2 * d.H; k.max_voxels = (u64)d.p.max_voxels; k.max_pairs = 2 * (u64)d.p.max_voxels;
  k.ctr = s.at<u64>(DB_CTR);
  ESL_HIP_TRY(hipMemsetAsync(k.ctr, 0, 5 * sizeof(u64), c->stream));   // this call's counts
  {
    ProfScope ps(c, 4);
    const dim3 grid(dense_blocks((u64)per), (unsigned)std::min(F, 65535));
    if (d.combine) hipLaunchKernelGGL(k_dense_insert<true>, grid, dim3(kDenseThreads), 0, c->stream, k);
    else hipLaunchKernelGGL(k_dense_insert<false>, grid, dim3(kDenseThreads), 0, c->stream, k);
  }
  ESL_HIP_TRY(hipGetLastError());
  u64 ctr[DC_COUNT];
  ESL_HIP_TRY(hipMemcpyAsync(ctr, k.ctr, sizeof(ctr), hipMemcpyDeviceToHost, c->stream));
  ESL_HIP_TRY(hipStreamSynchronize(c->stream));   // the caller's arrays are free again
  d.n_samples += (long long)ctr[DC_USED];
  d.n_voxels = (long long)ctr[DC_VOXELS]; d.n_pairs = (long long)ctr[DC_PAIRS];
  d.status = ctr[DC_STATUS] ? 3 : 0;
  if (out) {
    out->n_sampled = (int64_t)ctr[DC_SAMPLED]; out->n_zero = (int64_t)ctr[DC_ZERO]; out->n_depth_out = (int64_t)ctr[DC_DEPTH_OUT];
    out->n_key_out = (int64_t)ctr[DC_KEY_OUT]; out->n_used = (int64_t)ctr[DC_USED]; out->status = d.status; out->pad = 0;
  }
  return ESL_OK;
}

extern "C" int esl_dense_extract(esl_ctx* c, int64_t cap, int32_t* key_out, double* xyz_out, int32_t* count_out, uint8_t* bgr_out,
                                 int32_t* inst_out, int32_t* votes_out, int64_t* n_voxels) {
  const char* who = "esl_dense_extract";
  if (!c) return dense_fail(ESL_ERR_INVALID, who, "null ctx");
  if (cap < 0) return dense_fail(ESL_ERR_INVALID, who, "negative cap");
  if (!n_voxels) return dense_fail(ESL_ERR_INVALID, who, "null n_voxels");
  if (!c->dense || !c->dense->begun) return dense_fail(ESL_ERR_STATE, who, "no esl_dense_begin before");
  DenseState& d = *c->dense;
  if (d.status) { *n_voxels = -1; return ESL_OK; }   // over capacity: the map is invalid, nothing is written
  *n_voxels = d.n_voxels;
  const long long n = d.n_voxels, nw = std::min<long long>(n, cap);
  const bool any = key_out || xyz_out || count_out || bgr_out || inst_out || votes_out;
  if (nw == 0 || !any) return ESL_OK;
  ESL_HIP_TRY(hipSetDevice(c->device));
  ScratchSet<DB_COUNT>& s = d.set;
  DenseOutArgs k;
  std::memset(&k, 0, sizeof(k));
  if (const int rc = s.grow(c, DB_LKEY, (size_t)n * sizeof(u64))) return rc;
  if (const int rc = s.grow(c, DB_LVAL, (size_t)n * sizeof(unsigned int))) return rc;
  if (const int rc = s.grow(c, DB_SKEY, (size_t)n * sizeof(u64))) return rc;
  if (const int rc = s.grow(c, DB_SVAL, (size_t)n * sizeof(unsigned int))) return rc;
  size_t temp_bytes = 0;
  ESL_HIP_TRY(rocprim::radix_sort_pairs(nullptr, temp_bytes, s.at<u64>(DB_LKEY), s.at<u64>(DB_SKEY), s.at<unsigned int>(DB_LVAL),
                                        s.at<unsigned int>(DB_SVAL), (size_t)n, 0, 63, c->stream));
  if (const int rc = s.grow(c, DB_TEMP, temp_bytes)) return rc;
  if (key_out) { if (const int rc = s.grow(c, DB_OKEY, (size_t)nw * 3 * sizeof(int32_t))) return rc; k.okey = s.at<int>(DB_OKEY); }
  if (xyz_out) { if (const int rc = s.grow(c, DB_OXYZ, (size_t)nw * 3 * sizeof(double))) return rc; k.oxyz = s.at<double>(DB_OXYZ); }
  if (count_out) { if (const int rc = s.grow(c, DB_OCNT, (size_t)nw * sizeof(int32_t))) return rc; k.ocnt = s.at<int>(DB_OCNT); }
  if (bgr_out) { if (const int rc = s.grow(c, DB_OBGR, (size_t)nw * 3)) return rc; k.obgr = s.at<unsigned char>(DB_OBGR); }
  if (inst_out) { if (const int rc = s.grow(c, DB_OINST, (size_t)nw * sizeof(int32_t))) return rc; k.oinst = s.at<int>(DB_OINST); }
  if (votes_out) { if (const int rc = s.grow(c, DB_OVOTES, (size_t)nw * sizeof(int32_t))) return rc; k.ovotes = s.at<int>(DB_OVOTES); }
  k.keys = s.at<u64>(DB_KEYS); k.rec = s.at<DenseRec>(DB_REC);
  k.H = d.H; k.P = 2 * d.H; k.ctr = s.at<u64>(DB_CTR);
  k.lkey = s.at<u64>(DB_LKEY); k.lval = s.at<unsigned int>(DB_LVAL); k.list_cap = (u64)n;
  k.skey = s.at<u64>(DB_SKEY); k.sval = s.at<unsigned int>(DB_SVAL); k.n_write = nw;
  k.with_color = d.with_color;
  const bool vote = d.with_inst && (inst_out || votes_out);
  if (vote) { k.pkeys = s.at<u64>(DB_PKEYS); k.pcnt = s.at<unsigned int>(DB_PCNT); }
  ESL_HIP_TRY(hipMemsetAsync(k.ctr + DC_LIST, 0, sizeof(u64), c->stream));
  {
    ProfScope ps(c, 4);
    hipLaunchKernelGGL(k_dense_compact, dim3(dense_blocks(k.H)), dim3(kDenseThreads), 0, c->stream, k);
    if (vote) hipLaunchKernelGGL(k_dense_vote, dim3(dense_blocks(k.P)), dim3(kDenseThreads), 0, c->stream, k);
    ESL_HIP_TRY(rocprim::radix_sort_pairs(s.buf[DB_TEMP], temp_bytes, s.at<u64>(DB_LKEY), s.at<u64>(DB_SKEY),
                                          s.at<unsigned int>(DB_LVAL), s.at<unsigned int>(DB_SVAL), (size_t)n, 0, 63, c->stream));
    hipLaunchKernelGGL(k_dense_gather, dim3(dense_blocks((u64)nw)), dim3(kDenseThreads), 0, c->stream, k);
  }
  ESL_HIP_TRY(hipGetLastError());
  if (key_out) ESL_HIP_TRY(hipMemcpyAsync(key_out, k.okey, (size_t)nw * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  if (xyz_out) ESL_HIP_TRY(hipMemcpyAsync(xyz_out, k.oxyz, (size_t)nw * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (count_out) ESL_HIP_TRY(hipMemcpyAsync(count_out, k.ocnt, (size_t)nw * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  if (bgr_out) ESL_HIP_TRY(hipMemcpyAsync(bgr_out, k.obgr, (size_t)nw * 3, hipMemcpyDeviceToHost, c->stream));
  if (inst_out) ESL_HIP_TRY(hipMemcpyAsync(inst_out, k.oinst, (size_t)nw * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  if (votes_out) ESL_HIP_TRY(hipMemcpyAsync(votes_out, k.ovotes, (size_t)nw * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  ESL_HIP_TRY(hipStreamSynchronize(c->stream));
  return ESL_OK;
}
