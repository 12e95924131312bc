// esl_graph_layout.hpp — the rules that lay a graph out in device memory, host-only and written once.
//
// esl_graph_upload, the appendable layout of esl_graph_append (compact or with slack behind every ellipsoid's slice), its
// SLAM-mode camera tables and esl_graph_upload_fixed all build their arrays with these helpers (esl_graph.hip), which is
// what keeps "an append produces the order an upload of the whole graph would" true.  Standard library only: no HIP
// header, no esl_ctx (tests/graph_layout_main.cpp compiles it with a plain C++ compiler).  The helpers write through
// pointers the caller supplies -- esl_graph_upload hands them blocks of its pinned staging blob.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace esl {
namespace layout {

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Counting sort into a CSR, written once: walk(f) calls f(key, value) for every entry, twice in the same order; start[k] ..
// start[k + 1] then holds the values of key k in the order walk gave them (stable).  pos: scratch.
template <class Walk>
inline void csr_build(int n_keys, int* start, int* out, std::vector<int>& pos, Walk&& walk) {
  std::fill(start, start + n_keys + 1, 0);
  walk([&](int key, int) { start[(size_t)key + 1]++; });
  for (int k = 0; k < n_keys; ++k) start[(size_t)k + 1] += start[k];
  pos.assign(start, start + n_keys);
  walk([&](int key, int value) { out[(size_t)pos[key]++] = value; });
}
// perm = the indices 0 .. n - 1 sorted by key, stable
inline void csr_by_key(const int32_t* key, int n, int n_keys, int* start, int* perm, std::vector<int>& pos) {
  csr_build(n_keys, start, perm, pos, [&](auto&& f) { for (int i = 0; i < n; ++i) f(key[i], i); });
}
inline void csr_by_key(const int32_t* key, int n, int n_keys, std::vector<int>& start, std::vector<int>& perm) {
  std::vector<int> pos;
  start.resize((size_t)n_keys + 1);
  perm.resize((size_t)n);
  csr_by_key(key, n, n_keys, start.data(), perm.data(), pos);
}

// Per-ellipsoid ranges [begin(o), end(o)) of positions in an ellipsoid-sorted edge array: the compact form of an upload
// (start[o], start[o + 1]) or the slices of the appendable layout (begin[o], begin[o] + cnt[o]; slack behind them).
struct Ranges {
  const int* b; const int* cnt;   // cnt null: the compact form
  static Ranges csr(const int* start) { return {start, nullptr}; }
  static Ranges slices(const int* begin, const int* cnt) { return {begin, cnt}; }
  int begin(int o) const { return b[o]; }
  int end(int o) const { return cnt ? b[o] + cnt[o] : b[o + 1]; }
};

// ---- chunk table: per ellipsoid its bbox chunks (<= 64 edges) first, then its 3-D chunks (<= 32) ----
// upper bound of the chunk count of n_bbox / n_e3d edge slots on n_objs ellipsoids
inline size_t chunk_capacity(size_t n_bbox, size_t n_e3d, size_t n_objs) { return n_bbox / 64 + n_e3d / 32 + 2 * n_objs + 2; }
struct Chunks {   // obj .. end, ids_bb, ids_e3: room for chunk_capacity entries; ostart: n_objs + 1
  int *obj, *type, *begin, *end, *ids_bb, *ids_e3, *ostart;
  int n_chunks, n_ids_bb, n_ids_e3;
  static size_t ints(size_t cap, size_t n_objs) { return 6 * cap + n_objs + 1; }   // the seven arrays side by side in one block of ints
  static Chunks in(int* p, size_t cap) { return {p, p + cap, p + 2 * cap, p + 3 * cap, p + 4 * cap, p + 5 * cap, p + 6 * cap, 0, 0, 0}; }
};
inline void build_chunks(int n_objs, const Ranges& bb, const Ranges& e3, Chunks& t) {
  int n = 0;
  t.n_ids_bb = t.n_ids_e3 = 0;
  auto emit = [&](int o, int type, int b0, int b1) { t.obj[n] = o; t.type[n] = type; t.begin[n] = b0; t.end[n] = b1; return n++; };
  for (int o = 0; o < n_objs; ++o) {
    t.ostart[o] = n;
    for (int b = bb.begin(o), b1 = bb.end(o); b < b1; b += 64) t.ids_bb[t.n_ids_bb++] = emit(o, 0, b, std::min(b + 64, b1));
    for (int b = e3.begin(o), b1 = e3.end(o); b < b1; b += 32) t.ids_e3[t.n_ids_e3++] = emit(o, 1, b, std::min(b + 32, b1));
  }
  t.ostart[n_objs] = t.n_chunks = n;
}

// ---- appendable layout: the capacity of a slice that holds cnt edges (doubled, + one chunk, whole chunks) ----
inline size_t bbox_slice_capacity(size_t cnt) { return align_up(2 * cnt + 64, 64); }
inline size_t e3d_slice_capacity(size_t cnt) { return align_up(2 * cnt + 32, 32); }

// ---- cameras ----
// A free camera only enters the system if it has an active edge (sparse_optimizer.cpp:236-257): a bbox or 3-D edge, an
// odometry edge whose other end is not fixed too, or -- extra_touched, n_cams flags or null -- an edge the caller keeps
// elsewhere (the anchored edges of esl_graph_upload_fixed).  fixed: n_cams flags, 0 / 1.  Writes slot[n_cams] (index
// among the free cameras, or -1) and returns their number.
inline int free_camera_slots(int n_cams, const unsigned char* fixed, int n_objs, const int32_t* bb_cam, const Ranges& bb, const int32_t* e3_cam,
                             const Ranges& e3, int n_odom, const int32_t* od_i, const int32_t* od_j, const unsigned char* extra_touched, int* slot) {
  std::vector<unsigned char> touched((size_t)n_cams, 0);
  for (int o = 0; o < n_objs; ++o) {
    for (int k = bb.begin(o), k1 = bb.end(o); k < k1; ++k) touched[bb_cam[k]] = 1;
    for (int k = e3.begin(o), k1 = e3.end(o); k < k1; ++k) touched[e3_cam[k]] = 1;
  }
  for (int i = 0; i < n_odom; ++i)
    if (!(fixed[od_i[i]] && fixed[od_j[i]])) { touched[od_i[i]] = 1; touched[od_j[i]] = 1; }
  int nf = 0;
  for (int i = 0; i < n_cams; ++i) slot[i] = !fixed[i] && (touched[i] || (extra_touched && extra_touched[i])) ? nf++ : -1;
  return nf;
}

// camera-side CSR over the edges at the positions of r: start[n_cams + 1]; edge[] = the positions, ascending inside a
// camera's list -- ellipsoids ascend, arrival order holds inside one, so the camera blocks are summed in the order an
// upload of the whole graph gives (pos: scratch)
inline void camera_csr(int n_cams, int n_objs, const int32_t* cam, const Ranges& r, int* start, int* edge, std::vector<int>& pos) {
  csr_build(n_cams, start, edge, pos, [&](auto&& f) {
    for (int o = 0; o < n_objs; ++o)
      for (int k = r.begin(o), k1 = r.end(o); k < k1; ++k) f(cam[k], k);
  });
}
// camera-side CSR over the odometry edges: start[n_cams + 1]; edge[2 n_odom], entry = edge * 2 + side, ascending
inline void odometry_csr(int n_cams, int n_odom, const int32_t* od_i, const int32_t* od_j, int* start, int* edge, std::vector<int>& pos) {
  csr_build(n_cams, start, edge, pos, [&](auto&& f) { for (int e = 0; e < n_odom; ++e) { f(od_i[e], 2 * e); f(od_j[e], 2 * e + 1); } });
}

// ---- edge records ----
// one edge class as parallel arrays: camera, ellipsoid, weight, `width` measurements per edge (bbox 4, 3-D 10)
struct EdgeView { const int32_t* cam; const int32_t* obj; const double* meas; const double* w; int width; };
struct EdgeSet {
  int32_t* cam; int32_t* obj; double* meas; double* w; int width;
  operator EdgeView() const { return {cam, obj, meas, w, width}; }
};
inline void copy_edge(const EdgeSet& dst, size_t k, const EdgeView& src, size_t i) {
  dst.cam[k] = src.cam[i]; dst.obj[k] = src.obj[i]; dst.w[k] = src.w[i];
  if (src.width == 4) std::memcpy(dst.meas + k * 4, src.meas + i * 4, 4 * sizeof(double));   // constant sizes: the copies stay inline
  else std::memcpy(dst.meas + k * 10, src.meas + i * 10, 10 * sizeof(double));               // (the gather of an upload is this loop)
}

}  // namespace layout
}  // namespace esl
