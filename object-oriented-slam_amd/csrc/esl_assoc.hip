// esl_assoc.hip — esl_predict_boxes / esl_associate_boxes: 2-D data association of detection boxes against the projected map, given
// the poses (include/esl.h, "2-D data association").  One workgroup per frame (k_assoc_frames):
//   phase A  threads stride over the map; the bbox edge's own predicate and projection (esl_math.hpp bbox_edge_visible, box_geom,
//            box_from_conic) decide eligibility; the eligible predictions (clipped box, z, m, label) are compacted into a tile in LDS,
//            in ascending m (ballot per wave + the four wave counts)
//   phase B  occlusion: every tile entry against every other, O(V^2), stops at the first occluder
//   phase C  assignment: one detection at a time, every thread scores its share of the tile, a wave then a workgroup argmax on the
//            key (IoU descending, m ascending); the thread that owns the winning entry claims it
// A frame with more than kAssocTile eligible predictions is put on a list instead; a second launch (k_assoc_spilled) walks the list,
// as many frames at a time as a bounded global scratch has slices, with phase A writing into the slice and phases B and C reading it:
// the same code through other pointers, so the same bits.
// No floating-point atomics; every choice is a total order, so no result depends on the compaction order.
// Everything lives in buffers of its own (esl_ctx::assoc) on the context's stream; the resident graph is only read.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "esl_ctx.hpp"

namespace esl {

static_assert(sizeof(esl_assoc_params) == 32, "include/esl.h states this size");
// 1,024 entries of 52 bytes: 52 KB of LDS, three workgroups of 256 threads per CU (160 KB) -- phase C is a chain of barriers
// per detection, which other resident workgroups hide
constexpr int kAssocTile = 1024;
constexpr int kAssocThreads = 256;
constexpr size_t kAssocEntryBytes = 52;
constexpr size_t kAssocScratchBytes = 64ull << 20;   // of overflow tiles, unless one frame's slice alone is larger

struct AssocTile {
  double2* lo; double2* hi;   // (x1, y1), (x2, y2) of the clipped box
  double* z;
  int* m; int* lab;
  int* st;                    // bit 0 occluded, bit 1 claimed
};

struct AssocArgs {
  const double* cams; const double* objs; const int* obj_lab;
  int M;
  double K[4];
  int rows, cols;
  const int* det_off; const double* det_box; const int* det_lab;
  double min_iou, occl_ratio, min_box;
  int match_labels, occlusion;
  int* assoc; double* iou; int* stats;
  double* p_box; double* p_depth; int* p_flags;   // esl_predict_boxes: per-object outputs of frame 0, else null
  char* scratch; size_t slice;                    // slices of the overflow tiles, one per workgroup of k_assoc_spilled
  int* spill_list; int* spill_count;              // the frames left to k_assoc_spilled (all null when M <= kAssocTile)
};

enum { AB_CAMS, AB_OBJS, AB_OLAB, AB_OFF, AB_DBOX, AB_DLAB, AB_ASSOC, AB_IOU, AB_STATS, AB_PBOX, AB_PDEPTH, AB_PFLAGS, AB_SCRATCH, AB_SPILL,
       AB_COUNT };
struct AssocState { ScratchSet<AB_COUNT> set; };

static __device__ __forceinline__ AssocTile assoc_tile_at(char* base, size_t cap) {
  AssocTile t;
  t.lo = (double2*)base; t.hi = (double2*)(base + 16 * cap); t.z = (double*)(base + 32 * cap);
  t.m = (int*)(base + 40 * cap); t.lab = (int*)(base + 44 * cap); t.st = (int*)(base + 48 * cap);
  return t;
}

static __device__ __forceinline__ double assoc_overlap(double2 alo, double2 ahi, double2 blo, double2 bhi) {
  const double w = fmin(ahi.x, bhi.x) - fmax(alo.x, blo.x), h = fmin(ahi.y, bhi.y) - fmax(alo.y, blo.y);
  return (w > 0 && h > 0) ? w * h : 0.0;
}

// phase A: step 1 for every map object, the eligible ones to tile[0 .. min(V, cap)) in ascending m; returns V (workgroup-uniform)
static __device__ __forceinline__ int assoc_project(const AssocArgs& a, const SE3& Tcw, const AssocTile& t, int cap, int* s_cnt) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const double qnan = __builtin_nan("");
  int base = 0, it = 0;
  for (int m0 = 0; m0 < a.M; m0 += kAssocThreads, ++it) {
    const int m = m0 + tid;
    bool ok = false;
    double c[4] = {qnan, qnan, qnan, qnan}, z = qnan;
    if (m < a.M) {
      const Ell e = ell_load(a.objs + (size_t)m * 10);
      if (bbox_edge_visible(Tcw, e, a.K, a.rows, a.cols)) {
        BoxGeom g;
        box_geom(Tcw, e, a.K, g);
        double bb[4], sq[2];
        box_from_conic(g, bb, sq);
        if (isfinite(bb[0]) && isfinite(bb[1]) && isfinite(bb[2]) && isfinite(bb[3])) {
          const double x1 = fmax(bb[0], 0.0), y1 = fmax(bb[1], 0.0), x2 = fmin(bb[2], (double)a.cols), y2 = fmin(bb[3], (double)a.rows);
          if (x2 - x1 >= a.min_box && y2 - y1 >= a.min_box) {
            ok = true;
            c[0] = x1; c[1] = y1; c[2] = x2; c[3] = y2; z = g.n[3][2];
          }
        }
      }
      if (a.p_box) {
        double* pb = a.p_box + (size_t)m * 4;
        pb[0] = c[0]; pb[1] = c[1]; pb[2] = c[2]; pb[3] = c[3];
        a.p_depth[m] = z; a.p_flags[m] = ok ? 1 : 0;
      }
    }
    const unsigned long long mask = __ballot(ok);
    int* cnt = s_cnt + (it & 1) * 4;      // two sets: the next round's counts do not wait for this round's readers
    if (lane == 0) cnt[wv] = __popcll(mask);
    __syncthreads();
    int off = base;
    for (int w = 0; w < 4; ++w) { const int n = cnt[w]; if (w < wv) off += n; base += n; }
    if (ok) {
      const int pos = off + __popcll(mask & ((1ull << lane) - 1ull));
      if (pos < cap) {
        t.lo[pos] = make_double2(c[0], c[1]); t.hi[pos] = make_double2(c[2], c[3]); t.z[pos] = z;
        t.m[pos] = m; t.lab[pos] = a.obj_lab ? a.obj_lab[m] : 0; t.st[pos] = 0;
      }
    }
  }
  __syncthreads();
  return base;
}

// phases B and C on a tile of V entries
static __device__ __forceinline__ void assoc_frame(const AssocArgs& a, int f, const AssocTile& t, int V, int spilled, int* s_nocc,
                                                   double* s_iou, int* s_key) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (a.occlusion) {
    for (int i = tid; i < V; i += kAssocThreads) {
      const double2 lo = t.lo[i], hi = t.hi[i];
      const double zi = t.z[i], need = a.occl_ratio * ((hi.x - lo.x) * (hi.y - lo.y));
      const int mi = t.m[i];
      bool hid = false;
      // four entries per round, no branch inside: their LDS reads are in flight together; a repeat of the last entry changes nothing
      for (int j0 = 0; j0 < V && !hid; j0 += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int j = min(j0 + u, V - 1);
          const double zj = t.z[j];
          const bool nearer = j != i && (zj < zi || (zj == zi && t.m[j] < mi));
          hid |= nearer & (assoc_overlap(lo, hi, t.lo[j], t.hi[j]) >= need);
        }
      }
      if (hid) {
        t.st[i] = 1;
        atomicAdd(s_nocc, 1);
        if (a.p_flags) a.p_flags[mi] = 3;
      }
    }
  }
  __syncthreads();
  int n_assigned = 0, it = 0;
  const int d0 = a.det_off[f], d1 = a.det_off[f + 1];
  for (int d = d0; d < d1; ++d) {
    const double* db = a.det_box + (size_t)d * 4;
    const double x1 = db[0], y1 = db[1], x2 = db[2], y2 = db[3];
    int win = -1; double win_iou = 0;
    const bool valid = isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2) && x2 > x1 && y2 > y1;
    if (valid && V > 0) {   // workgroup-uniform
      const int dl = a.match_labels ? a.det_lab[d] : 0;
      const double2 dlo = make_double2(x1, y1), dhi = make_double2(x2, y2);
      const double da = (x2 - x1) * (y2 - y1);
      double b_iou = -1.0; int b_m = 0x7fffffff, b_i = -1;
      for (int i = tid; i < V; i += kAssocThreads) {
        if (t.st[i] != 0 || (a.match_labels && t.lab[i] != dl)) continue;
        const double2 lo = t.lo[i], hi = t.hi[i];
        const double in = assoc_overlap(dlo, dhi, lo, hi);
        const double iou = in / (da + (hi.x - lo.x) * (hi.y - lo.y) - in);
        const int m = t.m[i];
        if (iou > b_iou || (iou == b_iou && m < b_m)) { b_iou = iou; b_m = m; b_i = i; }
      }
      for (int off = 32; off > 0; off >>= 1) {
        const double u2 = __shfl_xor(b_iou, off, 64);
        const int m2 = __shfl_xor(b_m, off, 64), i2 = __shfl_xor(b_i, off, 64);
        if (u2 > b_iou || (u2 == b_iou && m2 < b_m)) { b_iou = u2; b_m = m2; b_i = i2; }
      }
      double* r_iou = s_iou + (it & 1) * 4; int* r_key = s_key + (it & 1) * 8;   // two sets: one barrier per detection
      ++it;
      if (lane == 0) { r_iou[wv] = b_iou; r_key[wv * 2] = b_m; r_key[wv * 2 + 1] = b_i; }
      __syncthreads();
      b_iou = r_iou[0]; b_m = r_key[0]; b_i = r_key[1];
      for (int w = 1; w < 4; ++w) {
        const double u2 = r_iou[w]; const int m2 = r_key[w * 2];
        if (u2 > b_iou || (u2 == b_iou && m2 < b_m)) { b_iou = u2; b_m = m2; b_i = r_key[w * 2 + 1]; }
      }
      if (b_i >= 0 && b_iou >= a.min_iou && b_iou > 0) {
        win = b_m; win_iou = b_iou; ++n_assigned;
        if ((b_i & (kAssocThreads - 1)) == tid) t.st[b_i] = 2;   // the one thread that reads this entry again
      }
    }
    if (tid == 0) {
      a.assoc[d] = win;
      if (a.iou) a.iou[d] = win_iou;
    }
  }
  if (tid == 0 && a.stats) {
    int* s = a.stats + (size_t)f * 4;
    s[0] = V; s[1] = *s_nocc; s[2] = n_assigned; s[3] = spilled;
  }
}

// grid = frames.  A frame whose eligible predictions overflow the tile is put on the spill list (integer atomic: the order of the list
// is free, a frame's result does not depend on its place) and left to k_assoc_spilled.
static __global__ __launch_bounds__(kAssocThreads) void k_assoc_frames(AssocArgs a) {
  __shared__ __attribute__((aligned(16))) char s_tile[kAssocTile * kAssocEntryBytes];
  __shared__ int s_cnt[8], s_key[16], s_nocc;
  __shared__ double s_iou[8];
  const int f = blockIdx.x;
  if (threadIdx.x == 0) s_nocc = 0;
  const SE3 Tcw = se3_load(a.cams + (size_t)f * 7);
  const AssocTile lt = assoc_tile_at(s_tile, kAssocTile);
  const int V = assoc_project(a, Tcw, lt, kAssocTile, s_cnt);
  if (V <= kAssocTile) assoc_frame(a, f, lt, V, 0, &s_nocc, s_iou, s_key);
  else if (threadIdx.x == 0) a.spill_list[atomicAdd(a.spill_count, 1)] = f;   // only when M > kAssocTile: the list exists
}

// grid = slices of the scratch.  Every workgroup walks the spill list with the grid's stride, the frame's tile in its own slice
// (M entries: every object of the map fits).
static __global__ __launch_bounds__(kAssocThreads) void k_assoc_spilled(AssocArgs a) {
  __shared__ int s_cnt[8], s_key[16], s_nocc;
  __shared__ double s_iou[8];
  const AssocTile gt = assoc_tile_at(a.scratch + (size_t)blockIdx.x * a.slice, (size_t)a.M);
  const int n = *a.spill_count;
  for (int k = blockIdx.x; k < n; k += gridDim.x) {
    __syncthreads();   // the frame before is finished with the counters
    if (threadIdx.x == 0) s_nocc = 0;
    const int f = a.spill_list[k];
    const SE3 Tcw = se3_load(a.cams + (size_t)f * 7);
    const int V = assoc_project(a, Tcw, gt, a.M, s_cnt);
    assoc_frame(a, f, gt, V, 1, &s_nocc, s_iou, s_key);
  }
}

void assoc_scratch_stats(const esl_ctx* c, int64_t* allocs, int64_t* bytes) {
  if (c->assoc) { *allocs = c->assoc->set.allocs(); *bytes = (int64_t)c->assoc->set.held(); }
}

void assoc_release(esl_ctx* c) {   // called by esl_ctx_destroy
  if (c->assoc) c->assoc->set.release();
  delete c->assoc;
  c->assoc = nullptr;
}

}  // namespace esl

using namespace esl;

namespace {

struct AssocCall {
  const double* cams; int F;             // host, or null = resident
  const double* objs; const int32_t* obj_labels; int M;
  const double* K; int rows, cols;
  const int32_t* det_off; const double* det_boxes; const int32_t* det_labels;   // null offsets: no detections (esl_predict_boxes)
  const esl_assoc_params* p;
  int32_t* assoc_out; double* iou_out; int32_t* stats_out;
  double* boxes_out; double* depth_out; int32_t* flags_out;
};

// the checks both calls share; fills p
int assoc_check(esl_ctx* c, const AssocCall& a, const char* who, esl_assoc_params& p) {
  const std::string w(who);
  if (!c || a.F < 0 || a.M < 0 || !a.K) { set_error(w + ": bad argument (null pointer or negative count)"); return ESL_ERR_INVALID; }
  if (a.rows < 1 || a.cols < 1) { set_error(w + ": rows or cols < 1"); return ESL_ERR_INVALID; }
  if (a.p) p = *a.p; else esl_assoc_params_default(&p);
  for (double v : {p.min_iou, p.occl_ratio, p.min_box_px})
    if (!std::isfinite(v) || v < 0) { set_error(w + ": non-finite or negative min_iou / occl_ratio / min_box_px"); return ESL_ERR_INVALID; }
  return resident_source_check(c, who, !a.cams && a.F > 0, a.F, !a.objs && a.M > 0, a.M);
}

int assoc_run(esl_ctx* c, const AssocCall& a, const esl_assoc_params& p) {
  ESL_HIP_TRY(hipSetDevice(c->device));
  if (!c->assoc) c->assoc = new AssocState();
  ScratchSet<AB_COUNT>& s = c->assoc->set;
  const int F = a.F, M = a.M;
  const size_t n_det = a.det_off ? (size_t)a.det_off[F] : 0;
  const bool predict = a.boxes_out != nullptr;
  AssocArgs k;
  std::memset(&k, 0, sizeof(k));
  if (const int rc = source(c, s, AB_CAMS, a.cams, c->cams, (size_t)F * 7 * sizeof(double), &k.cams)) return rc;
  if (const int rc = source(c, s, AB_OBJS, a.objs, c->objs, (size_t)M * 10 * sizeof(double), &k.objs)) return rc;
  if (a.obj_labels)
    if (const int rc = upload(c, s, AB_OLAB, a.obj_labels, (size_t)M * sizeof(int32_t), &k.obj_lab)) return rc;
  // offsets (zeros when there are no detections at all), boxes, labels
  if (const int rc = s.grow(c, AB_OFF, (size_t)(F + 1) * sizeof(int32_t))) return rc;
  if (a.det_off) ESL_HIP_TRY(hipMemcpyAsync(s.buf[AB_OFF], a.det_off, (size_t)(F + 1) * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  else ESL_HIP_TRY(hipMemsetAsync(s.buf[AB_OFF], 0, (size_t)(F + 1) * sizeof(int32_t), c->stream));
  k.det_off = s.at<int>(AB_OFF);
  if (const int rc = s.grow(c, AB_DBOX, n_det * 4 * sizeof(double))) return rc;
  if (const int rc = s.grow(c, AB_DLAB, n_det * sizeof(int32_t))) return rc;
  if (const int rc = s.grow(c, AB_ASSOC, n_det * sizeof(int32_t))) return rc;
  if (n_det) {
    ESL_HIP_TRY(hipMemcpyAsync(s.buf[AB_DBOX], a.det_boxes, n_det * 4 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    ESL_HIP_TRY(hipMemcpyAsync(s.buf[AB_DLAB], a.det_labels, n_det * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  }
  k.det_box = s.at<double>(AB_DBOX); k.det_lab = s.at<int>(AB_DLAB); k.assoc = s.at<int>(AB_ASSOC);
  if (a.iou_out) {
    if (const int rc = s.grow(c, AB_IOU, n_det * sizeof(double))) return rc;
    k.iou = s.at<double>(AB_IOU);
  }
  if (a.stats_out) {
    if (const int rc = s.grow(c, AB_STATS, (size_t)F * 4 * sizeof(int32_t))) return rc;
    k.stats = s.at<int>(AB_STATS);
  }
  if (predict) {
    if (const int rc = s.grow(c, AB_PBOX, (size_t)M * 4 * sizeof(double))) return rc;
    if (const int rc = s.grow(c, AB_PDEPTH, (size_t)M * sizeof(double))) return rc;
    if (const int rc = s.grow(c, AB_PFLAGS, (size_t)M * sizeof(int32_t))) return rc;
    k.p_box = s.at<double>(AB_PBOX); k.p_depth = s.at<double>(AB_PDEPTH); k.p_flags = s.at<int>(AB_PFLAGS);
  }
  // frames that overflow the tile (possible only when M > kAssocTile) go on a list; as many of them at a time as the scratch bound
  // admits slices run in a second launch (at least one)
  int n_slices = 0;
  if (M > kAssocTile) {
    k.slice = ((size_t)M * kAssocEntryBytes + 15) / 16 * 16;
    n_slices = (int)std::max<size_t>(1, std::min<size_t>((size_t)F, kAssocScratchBytes / k.slice));
    if (const int rc = s.grow(c, AB_SCRATCH, k.slice * (size_t)n_slices)) return rc;
    if (const int rc = s.grow(c, AB_SPILL, (size_t)(F + 1) * sizeof(int))) return rc;
    k.scratch = s.at<char>(AB_SCRATCH);
    k.spill_count = s.at<int>(AB_SPILL); k.spill_list = k.spill_count + 1;
    ESL_HIP_TRY(hipMemsetAsync(k.spill_count, 0, sizeof(int), c->stream));
  }
  k.M = M; k.rows = a.rows; k.cols = a.cols;
  for (int i = 0; i < 4; ++i) k.K[i] = a.K[i];
  k.min_iou = p.min_iou; k.occl_ratio = p.occl_ratio; k.min_box = p.min_box_px;
  k.match_labels = p.match_labels != 0; k.occlusion = p.occlusion != 0;
  {
    ProfScope ps(c, 4);
    hipLaunchKernelGGL(k_assoc_frames, dim3((unsigned)F), dim3(kAssocThreads), 0, c->stream, k);
    if (n_slices) hipLaunchKernelGGL(k_assoc_spilled, dim3((unsigned)n_slices), dim3(kAssocThreads), 0, c->stream, k);
  }
  ESL_HIP_TRY(hipGetLastError());
  if (n_det) ESL_HIP_TRY(hipMemcpyAsync(a.assoc_out, k.assoc, n_det * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  if (n_det && a.iou_out) ESL_HIP_TRY(hipMemcpyAsync(a.iou_out, k.iou, n_det * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (a.stats_out) ESL_HIP_TRY(hipMemcpyAsync(a.stats_out, k.stats, (size_t)F * 4 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  if (predict) {
    ESL_HIP_TRY(hipMemcpyAsync(a.boxes_out, k.p_box, (size_t)M * 4 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    ESL_HIP_TRY(hipMemcpyAsync(a.depth_out, k.p_depth, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    ESL_HIP_TRY(hipMemcpyAsync(a.flags_out, k.p_flags, (size_t)M * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  }
  ESL_HIP_TRY(hipStreamSynchronize(c->stream));   // the caller's arrays are free again, the outputs filled
  return ESL_OK;
}

}  // namespace

extern "C" void esl_assoc_params_default(esl_assoc_params* p) {
  if (!p) return;
  p->min_iou = 0.3; p->occl_ratio = 0.7; p->min_box_px = 10.0; p->match_labels = 1; p->occlusion = 1;
}

extern "C" int esl_predict_boxes(esl_ctx* c, const double Tcw[7], const double* objs, int32_t M, const double K[4], int32_t rows,
                                 int32_t cols, const esl_assoc_params* pp, double* boxes_out, double* depth_out, int32_t* flags_out) {
  AssocCall a;
  std::memset(&a, 0, sizeof(a));
  a.cams = Tcw; a.F = 1; a.objs = objs; a.M = M; a.K = K; a.rows = rows; a.cols = cols; a.p = pp;
  a.boxes_out = boxes_out; a.depth_out = depth_out; a.flags_out = flags_out;
  if (!Tcw || (M > 0 && (!boxes_out || !depth_out || !flags_out))) { set_error("esl_predict_boxes: null pointer"); return ESL_ERR_INVALID; }
  esl_assoc_params p;
  if (const int rc = assoc_check(c, a, "esl_predict_boxes", p)) return rc;
  if (M == 0) return ESL_OK;
  return assoc_run(c, a, p);
}

extern "C" int esl_associate_boxes(esl_ctx* c, const double* cams, int32_t F, const double* objs, const int32_t* obj_labels, int32_t M,
                                   const double K[4], int32_t rows, int32_t cols, const int32_t* det_offsets, const double* det_boxes,
                                   const int32_t* det_labels, const esl_assoc_params* pp, int32_t* assoc_out, double* iou_out,
                                   int32_t* frame_stats_out) {
  AssocCall a;
  std::memset(&a, 0, sizeof(a));
  a.cams = cams; a.F = F; a.objs = objs; a.obj_labels = obj_labels; a.M = M; a.K = K; a.rows = rows; a.cols = cols;
  a.det_off = det_offsets; a.det_boxes = det_boxes; a.det_labels = det_labels; a.p = pp;
  a.assoc_out = assoc_out; a.iou_out = iou_out; a.stats_out = frame_stats_out;
  esl_assoc_params p;
  if (const int rc = assoc_check(c, a, "esl_associate_boxes", p)) return rc;
  if (!det_offsets || (M > 0 && !obj_labels)) { set_error("esl_associate_boxes: null offsets or object labels"); return ESL_ERR_INVALID; }
  if (det_offsets[0] != 0) { set_error("esl_associate_boxes: det_offsets[0] is not 0"); return ESL_ERR_INVALID; }
  for (int f = 0; f < F; ++f)
    if (det_offsets[f + 1] < det_offsets[f]) { set_error("esl_associate_boxes: det_offsets decrease"); return ESL_ERR_INVALID; }
  const int32_t n_det = det_offsets[F];
  if (n_det > 0 && (!det_boxes || !det_labels || !assoc_out)) { set_error("esl_associate_boxes: null detection array"); return ESL_ERR_INVALID; }
  if (F == 0) return ESL_OK;
  if (M == 0) {   // nothing to project: every detection stays unassigned
    for (int32_t d = 0; d < n_det; ++d) { assoc_out[d] = -1; if (iou_out) iou_out[d] = 0; }
    if (frame_stats_out) std::memset(frame_stats_out, 0, (size_t)F * 4 * sizeof(int32_t));
    return ESL_OK;
  }
  return assoc_run(c, a, p);
}
