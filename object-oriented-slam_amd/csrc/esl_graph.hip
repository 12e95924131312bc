// esl_graph.hip — graph residency: what lays a graph out in device memory and keeps it there.  esl_graph_upload (compact
// layout, grow-only arenas), esl_graph_upload_fixed, the appendable layout of esl_graph_append with its host image, and the
// states.  The layout RULES -- chunk table, slice capacities, free-camera slots, camera-side lists, edge records -- are
// written once in esl_graph_layout.hpp; this file owns the staging, the device blobs and the context's bookkeeping.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "esl_graph_int.hpp"
#include "esl_graph_layout.hpp"
#include "esl_kernels_map.hpp"
#include "esl_slam.hpp"

using namespace esl;
using namespace esl::layout;

template <class T> static void forget(T** p) { *p = nullptr; }   // interior pointer of an arena

// ---- arenas ---------------------------------------------------------------------------------------
// Device pointers handed out by the stages are INTERIOR pointers of a grow-only blob (c->arena_graph, c->arena_work, ...): never
// hipFree()d one by one (free_graph only forgets them), the blobs grow and are released with the context.
int esl::arena_reserve(char** dev, size_t* cap, size_t need) {
  if (need <= *cap) return ESL_OK;
  if (*dev) { (void)hipFree(*dev); *dev = nullptr; *cap = 0; }
  const size_t want = need + need / 2 + 4096;
  ESL_HIP_TRY(hipMalloc((void**)dev, want));
  *cap = want;
  return ESL_OK;
}
// The one blob packer: arrays are packed, 256-byte aligned, straight into the context's pinned staging block (grown on demand,
// kept) and go to the device blob (dev, cap) the stage was made for; commit() points every registered pointer at its array.
// One stage at a time owns the staging block: its user synchronises the stream before the next one packs.
struct UploadStage {
  struct Fix { void** dst; size_t off; };
  esl_ctx* c;
  char** dev; size_t* cap;
  size_t used = 0, sent = 0;
  int err = ESL_OK; bool early = false;
  std::vector<Fix> fixes;
  UploadStage(esl_ctx* ctx, char** dev_blob, size_t* dev_cap) : c(ctx), dev(dev_blob), cap(dev_cap) {}
  bool reserve(size_t need) {
    if (need <= c->stage_host_cap) return true;
    const size_t want = std::max(need + need / 2 + 4096, 2 * c->stage_host_cap);
    char* nb = nullptr;
    if (hipHostMalloc((void**)&nb, want, hipHostMallocDefault) != hipSuccess) { esl::set_error("hipHostMalloc (upload staging) failed"); err = ESL_ERR_HIP; return false; }
    if (c->stage_host) { std::memcpy(nb, c->stage_host, used); (void)hipHostFree(c->stage_host); }
    c->stage_host = nb; c->stage_host_cap = want;
    return true;
  }
  // the caller fills the returned block itself (no intermediate copy); after begin() the block never moves
  template <class T>
  T* alloc(T** dst, size_t n) {
    const size_t off = align_up(used, 256), bytes = std::max<size_t>(n, 1) * sizeof(T);
    if (err || !reserve(off + bytes)) return nullptr;
    used = off + bytes;
    fixes.push_back({(void**)dst, off});
    return (T*)(c->stage_host + off);
  }
  template <class T>
  void add(T** dst, const T* src, size_t n) {
    T* at = alloc(dst, n);
    if (at && n) std::memcpy(at, src, n * sizeof(T));
  }
  // sizes both ends for `bound` bytes up front, so that flush() can ship finished sections while the host packs the next
  int begin(size_t bound) {
    if (!reserve(bound)) return err;
    if (int rc = arena_reserve(dev, cap, std::max<size_t>(bound, 256))) return err = rc;
    early = true;
    return ESL_OK;
  }
  int flush() {
    if (err) return err;
    if (!early || used > *cap) return ESL_OK;   // commit() ships everything
    return ship();
  }
  int commit() {
    if (err) return err;
    const size_t need = std::max<size_t>(used, 256);
    if (need > *cap) sent = 0;   // the blob moves: ship everything again
    int rc = arena_reserve(dev, cap, need);
    if (rc || (rc = ship())) return rc;
    for (const Fix& f : fixes) *f.dst = *dev + f.off;
    return ESL_OK;
  }
  int ship() {   // what has been packed since the last shipment
    if (used > sent) ESL_HIP_TRY(hipMemcpyAsync(*dev + sent, c->stage_host + sent, used - sent, hipMemcpyHostToDevice, c->stream));
    sent = used;
    return ESL_OK;
  }
};

// ---- the host image of the appendable layout (esl_graph_append) ------------------------------------
// The exact host copy of the device arrays: edges sorted by ellipsoid, every ellipsoid owning a slice [begin, begin + slice_cap)
// of which cnt entries are used.
namespace esl {
struct EdgeSlices {   // one edge class
  int width;          // measurements per edge: 4 (bbox) or 10 (3-D)
  size_t cap = 0, used = 0;   // slots of the arrays / extent the slices cover
  std::vector<int> begin, cnt, slice_cap, cam, obj;
  std::vector<double> meas, w;
  explicit EdgeSlices(int width_) : width(width_) {}
  EdgeSet set() { return {cam.data(), obj.data(), meas.data(), w.data(), width}; }
  EdgeView view() const { return {cam.data(), obj.data(), meas.data(), w.data(), width}; }
  Ranges ranges() const { return Ranges::slices(begin.data(), cnt.data()); }
  size_t slice_capacity(size_t n) const { return width == 4 ? bbox_slice_capacity(n) : e3d_slice_capacity(n); }
  int n_edges() const { int n = 0; for (int k : cnt) n += k; return n; }
  void resize(size_t n) { cam.resize(n); obj.resize(n); meas.resize(n * width); w.resize(n); }
  // start[o] = begin of ellipsoid o's slice, start[n_objs] = end of the laid-out extent (a real end sentinel: a kernel that walks
  // start[o] .. start[o + 1] sees the slice WITH its slack, whose slots carry obj = -1, weight 0 and -- bbox -- valid = 0)
  std::vector<int> starts(size_t len) const { std::vector<int> s(len, 0); std::copy(begin.begin(), begin.end(), s.begin()); s[begin.size()] = (int)used; return s; }
};
struct HostImage {
  bool appendable = false;          // the device arrays have this image's capacities
  int n_cams = 0, n_objs = 0, cap_cams = 0, cap_objs = 0, n_grav = 0, relayouts = 0;
  EdgeSlices bb{4}, e3{10};
  std::vector<int> gr_cnt;
  // SLAM mode: which cameras are fixed (empty = all of them) and the odometry edges
  std::vector<unsigned char> cam_fixed;
  std::vector<int> od_i, od_j;
  std::vector<double> od_meas, od_info;
  bool slam() const {
    if (!od_i.empty()) return true;
    for (unsigned char f : cam_fixed) if (!f) return true;
    return false;
  }
};
}  // namespace esl

// the flags of esl_graph_upload_fixed go away with the graph they belong to (the blob stays: grow-only)
static void fx_clear(esl_ctx* c) {
  c->fx_on = false;
  c->fx_flags.clear(); c->fx_bb_map.clear(); c->fx_e3_map.clear(); c->fx_grav_obj.clear();
  c->fx = AnchGraph{};
  c->fx_A = c->fx_chi = nullptr;
}

void esl::free_graph(esl_ctx* c) {
  DevGraph& g = c->g;
  delete c->append_img;   // the appendable host image describes the graph that goes away
  c->append_img = nullptr;
  (void)hipStreamSynchronize(c->stream);   // nothing may still read the arenas that are about to be rewritten
  forget(&g.bb_start); forget(&g.e3_start); forget(&g.gr_cnt);
  forget(&g.bb_cam); forget(&g.bb_obj); forget(&g.bb_meas); forget(&g.bb_w); forget(&g.bb_valid);
  forget(&g.e3_cam); forget(&g.e3_obj); forget(&g.e3_meas); forget(&g.e3_w);
  forget(&g.od_i); forget(&g.od_j); forget(&g.od_meas); forget(&g.od_info);
  forget(&g.cam_fixed); forget(&g.cam_slot);
  forget(&g.cbb_start); forget(&g.cbb_edge); forget(&g.ce3_start); forget(&g.ce3_edge);
  forget(&g.cod_start); forget(&g.cod_edge);
  forget(&c->ck_obj); forget(&c->ck_type); forget(&c->ck_begin); forget(&c->ck_end); forget(&c->ck_ostart);
  forget(&c->chunk_out); forget(&c->chunk_out2); forget(&c->chunk_chi); forget(&c->blk_part); forget(&c->solve_part); forget(&c->blk_chi);
  forget(&c->ck_ids_bb); forget(&c->ck_ids_e3);
  c->n_chunks = 0;
  forget(&c->cams); forget(&c->cams_trial); forget(&c->objs); forget(&c->objs_trial);
  forget(&c->Hoo); forget(&c->bo); forget(&c->xo); forget(&c->obj_part);
  // SLAM-mode tables and buffers are interior pointers of the context's grow-only blobs (esl_slam.hip): forgotten, not freed
  slam_forget(c);
  dev_free(&c->chol_pack); dev_free(&c->chol_pack2); c->chol_pack_len = 0;
  dev_free(&c->cams_snap); dev_free(&c->objs_snap);
  c->S_n = 0;
  c->graph_loaded = c->states_loaded = false;
  c->lm.begun = c->repl_checked = false;
}

// ---------------------------------------------------------------------------------------------------
// graph upload: validate, sort edges by ellipsoid (stable), build CSR
// ---------------------------------------------------------------------------------------------------
// order-independent structure fingerprint (comm_check_replicated): a 64-bit hash per edge / flag, summed
static inline unsigned long long fp_hash(unsigned long long a, unsigned long long b, unsigned long long c3) {
  unsigned long long h = 1469598103934665603ull;
  h = (h ^ a) * 1099511628211ull; h = (h ^ b) * 1099511628211ull; h = (h ^ c3) * 1099511628211ull;
  h ^= h >> 29; h *= 0xbf58476d1ce4e5b9ull; h ^= h >> 32;
  return h;
}
static unsigned long long fp_edges(int tag, int n, const int32_t* a, const int32_t* b) {
  unsigned long long s = 0;
  for (int i = 0; i < n; ++i) s += fp_hash((unsigned long long)tag, (unsigned)a[i], (unsigned)b[i]);
  return s;
}
static unsigned long long fp_fixed(int first_cam, int n, const uint8_t* fixed) {   // null = all fixed
  unsigned long long s = 0;
  for (int i = 0; i < n; ++i) s += fp_hash(4, (unsigned)(first_cam + i), fixed ? (fixed[i] ? 1u : 0u) : 1u);
  return s;
}
static EdgeView bbox_edges(const esl_graph* g) { return {g->bbox_cam, g->bbox_obj, g->bbox_meas, g->bbox_weight, 4}; }
static EdgeView e3d_edges(const esl_graph* g) { return {g->e3d_cam, g->e3d_obj, g->e3d_meas, g->e3d_weight, 10}; }
// every index of a graph's (who = "esl_graph") or a delta's ("esl_graph_delta") edges inside n_cams cameras / n_objs ellipsoids
static int check_indices(const char* who, int n_cams, int n_objs, const EdgeView& bb, int n_bbox, const EdgeView& e3, int n_e3d, const int32_t* grav_obj, int n_grav,
                         const int32_t* od_i, const int32_t* od_j, int n_odom) {
  auto in = [](int v, int n) { return v >= 0 && v < n; };
  auto bad = [&](const char* edges) { set_error(std::string(who) + ": " + edges + " edge index out of range"); return ESL_ERR_INVALID; };
  for (int i = 0; i < n_bbox; ++i) if (!in(bb.cam[i], n_cams) || !in(bb.obj[i], n_objs)) return bad("bbox");
  for (int i = 0; i < n_e3d; ++i) if (!in(e3.cam[i], n_cams) || !in(e3.obj[i], n_objs)) return bad("3-D");
  for (int i = 0; i < n_grav; ++i) if (!in(grav_obj[i], n_objs)) return bad("gravity");
  for (int i = 0; i < n_odom; ++i) if (!in(od_i[i], n_cams) || !in(od_j[i], n_cams)) return bad("odometry");
  return ESL_OK;
}
int esl::validate_graph(const esl_graph* g) {
  if (!g || g->n_cams < 0 || g->n_objs < 0 || g->n_bbox < 0 || g->n_e3d < 0 || g->n_grav < 0 || g->n_odom < 0) {
    set_error("esl_graph: null or negative size"); return ESL_ERR_INVALID;
  }
  if ((g->n_bbox && (!g->bbox_cam || !g->bbox_obj || !g->bbox_meas || !g->bbox_weight)) ||
      (g->n_e3d && (!g->e3d_cam || !g->e3d_obj || !g->e3d_meas || !g->e3d_weight)) ||
      (g->n_grav && !g->grav_obj) || (g->n_odom && (!g->odom_i || !g->odom_j || !g->odom_meas))) {
    set_error("esl_graph: null edge array with non-zero count"); return ESL_ERR_INVALID;
  }
  return check_indices("esl_graph", g->n_cams, g->n_objs, bbox_edges(g), g->n_bbox, e3d_edges(g), g->n_e3d, g->grav_obj, g->n_grav, g->odom_i, g->odom_j, g->n_odom);
}

// g: validated by the public entry.  extra_touched (n_cams flags or null): cameras that have an active edge outside g -- the
// anchored edges of esl_graph_upload_fixed
static int graph_upload_impl(esl_ctx* c, const esl_graph* g, const uint8_t* extra_touched) {
  const bool host_timing = std::getenv("ESL_UPLOAD_HOST_TIMING") != nullptr;   // diagnostic: where the host call's time goes
  auto now_us = [] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  double ht[16]; int nht = 0;
  auto mark = [&] { if (host_timing && nht < 16) ht[nht++] = now_us(); };
  mark();
  int rc;
  ESL_HIP_TRY(hipSetDevice(c->device));
  free_graph(c);
  c->graph_fp = fp_edges(1, g->n_bbox, g->bbox_cam, g->bbox_obj) + fp_edges(2, g->n_e3d, g->e3d_cam, g->e3d_obj) + fp_edges(3, g->n_odom, g->odom_i, g->odom_j) +
                fp_fixed(0, g->n_cams, g->cam_fixed);
  DevGraph& d = c->g;
  hipStream_t st = c->stream;
  // every array of the device-resident graph goes into ONE staging blob -> one H2D copy into a grow-only arena;
  // work buffers come from a second arena (a per-frame esl_optimize used to pay ~45 hipMalloc/hipFree pairs here)
  UploadStage up(c, &c->arena_graph, &c->arena_graph_cap);
  d.n_cams = g->n_cams; d.n_objs = g->n_objs; d.n_bbox = g->n_bbox; d.n_e3d = g->n_e3d; d.n_odom = g->n_odom;
  d.n_bbox_edges = g->n_bbox;
  d.K[0] = g->fx; d.K[1] = g->fy; d.K[2] = g->cx; d.K[3] = g->cy;
  d.grav_n[0] = g->grav_normal[0]; d.grav_n[1] = g->grav_normal[1]; d.grav_n[2] = g->grav_normal[2];
  d.grav_w = g->grav_weight;
  d.check_vis = g->check_visibility ? 1 : 0; d.img_rows = g->image_rows; d.img_cols = g->image_cols;
  {  // rotate_ellipsoid's yaw table (src/core/Ellipsoid.cpp:78, 100): yaw = k*pi/2, k = -1,0,1,2
    const double ang[4] = {-1, 0, 1, 2};
    double hs[4], hc[4];
    for (int k = 0; k < 4; ++k) { const double yaw = ang[k] * M_PI / 2.0; hs[k] = std::sin(yaw * 0.5); hc[k] = std::cos(yaw * 0.5); }
    yaw_table_fill(d.yt, hs, hc);
  }
  const int N = g->n_objs, F = g->n_cams;
  const size_t nb = (size_t)g->n_bbox, ne = (size_t)g->n_e3d, no = (size_t)g->n_odom;
  const size_t max_chunks = chunk_capacity(nb, ne, (size_t)N);
  {  // upper bound of the staging blob: lets finished sections go over PCIe while the host packs the next one
    auto blk = [](size_t n, size_t sz) { return align_up(std::max<size_t>(n, 1) * sz, 256) + 256; };
    const size_t bound = 3 * blk((size_t)N + 1, 4) + 3 * blk(nb, 4) + blk(nb * 4, 8) + blk(nb, 8) + blk(nb, 1) + 3 * blk((size_t)F + 1, 4) +
                         3 * blk(ne, 4) + blk(ne * 10, 8) + blk(ne, 8) + blk((size_t)N, 4) + 7 * blk(max_chunks, 4) + blk((size_t)F, 1) +
                         blk((size_t)F, 4) + 2 * blk(no, 4) + blk(no * 7, 8) + blk(no * 6, 8) + blk(no * 2, 4);
    if ((rc = up.begin(bound))) return rc;
  }
  std::vector<int> perm, perm3, pos, h_bb_start, h_e3_start;
  mark();   // 1: staging sized
  // edges are gathered in ellipsoid order straight into the pinned blob (C4: ~15 MB); the blob's edge arrays then go over
  // PCIe while the host builds the camera-side lists, the chunk table and the camera slots.  (Splitting the gather over
  // helper threads was measured and is not faster: profiles/r2_fused_experiments.txt)
  csr_by_key(g->bbox_obj, g->n_bbox, N, h_bb_start, perm);
  csr_by_key(g->e3d_obj, g->n_e3d, N, h_e3_start, perm3);
  const Ranges bb_ranges = Ranges::csr(h_bb_start.data()), e3_ranges = Ranges::csr(h_e3_start.data());
  int* b_start = up.alloc(&d.bb_start, (size_t)N + 1);
  const EdgeSet bb{up.alloc(&d.bb_cam, nb), up.alloc(&d.bb_obj, nb), up.alloc(&d.bb_meas, nb * 4), up.alloc(&d.bb_w, nb), 4};
  unsigned char* b_valid = up.alloc(&d.bb_valid, nb);
  int* e_start = up.alloc(&d.e3_start, (size_t)N + 1);
  const EdgeSet e3{up.alloc(&d.e3_cam, ne), up.alloc(&d.e3_obj, ne), up.alloc(&d.e3_meas, ne * 10), up.alloc(&d.e3_w, ne), 10};
  if (up.err) return up.err;
  std::copy(h_bb_start.begin(), h_bb_start.end(), b_start);
  std::copy(h_e3_start.begin(), h_e3_start.end(), e_start);
  mark();   // 2: both edge sets sorted by ellipsoid
  const EdgeView src_bb = bbox_edges(g), src_e3 = e3d_edges(g);
  for (size_t k = 0; k < nb; ++k) copy_edge(bb, k, src_bb, (size_t)perm[k]);
  if (nb) std::memset(b_valid, 1, nb);
  for (size_t k = 0; k < ne; ++k) copy_edge(e3, k, src_e3, (size_t)perm3[k]);
  mark();   // 3: gathered
  if ((rc = up.flush())) return rc;
  c->h_bb_cam.assign(bb.cam, bb.cam + nb); c->h_bb_obj.assign(bb.obj, bb.obj + nb);
  c->h_e3_cam.assign(e3.cam, e3.cam + ne); c->h_e3_obj.assign(e3.obj, e3.obj + ne);
  c->h_bb_slot_of.resize(nb); c->h_e3_slot_of.resize(ne);   // caller order -> slot (esl_edge_chi2)
  for (size_t k = 0; k < nb; ++k) c->h_bb_slot_of[perm[k]] = (int)k;
  for (size_t k = 0; k < ne; ++k) c->h_e3_slot_of[perm3[k]] = (int)k;
  {  // camera-side CSRs over the SORTED edges
    int* cs = up.alloc(&d.cbb_start, (size_t)F + 1);
    int* cp = up.alloc(&d.cbb_edge, nb);
    int* cs3 = up.alloc(&d.ce3_start, (size_t)F + 1);
    int* cp3 = up.alloc(&d.ce3_edge, ne);
    if (up.err) return up.err;
    camera_csr(F, N, bb.cam, bb_ranges, cs, cp, pos);
    camera_csr(F, N, e3.cam, e3_ranges, cs3, cp3, pos);
  }
  mark();   // 4: camera-side lists
  {  // gravity
    std::vector<int> cnt((size_t)N, 0);
    for (int i = 0; i < g->n_grav; ++i) cnt[g->grav_obj[i]]++;
    c->h_grav_obj.assign(g->grav_obj, g->grav_obj + g->n_grav);
    c->n_grav_edges = g->n_grav;
    for (int o = 0; o < N; ++o)
      if (cnt[o] > 64) { set_error("more than 64 gravity edges on one ellipsoid"); return ESL_ERR_INVALID; }
    up.add(&d.gr_cnt, cnt.data(), cnt.size());
    // chunk table: per ellipsoid, in g2o's edge order (gravity, bbox, 3-D)
    std::vector<int> tab(Chunks::ints(max_chunks, (size_t)N));
    Chunks t = Chunks::in(tab.data(), max_chunks);
    build_chunks(N, bb_ranges, e3_ranges, t);
    c->n_chunks = t.n_chunks; c->n_ids_bb = t.n_ids_bb; c->n_ids_e3 = t.n_ids_e3;
    up.add(&c->ck_obj, t.obj, (size_t)t.n_chunks); up.add(&c->ck_type, t.type, (size_t)t.n_chunks); up.add(&c->ck_begin, t.begin, (size_t)t.n_chunks);
    up.add(&c->ck_end, t.end, (size_t)t.n_chunks); up.add(&c->ck_ostart, t.ostart, (size_t)N + 1);
    up.add(&c->ck_ids_bb, t.ids_bb, (size_t)t.n_ids_bb); up.add(&c->ck_ids_e3, t.ids_e3, (size_t)t.n_ids_e3);
  }
  mark();   // 5: chunk table
  {  // cameras + odometry
    unsigned char* fixed = up.alloc(&d.cam_fixed, (size_t)F);
    int* slot = up.alloc(&d.cam_slot, (size_t)F);
    int* od_i = up.alloc(&d.od_i, no);
    int* od_j = up.alloc(&d.od_j, no);
    double* od_meas = up.alloc(&d.od_meas, no * 7);
    double* od_info = up.alloc(&d.od_info, no * 6);
    int* cs = up.alloc(&d.cod_start, (size_t)F + 1);
    int* cp = up.alloc(&d.cod_edge, no * 2);
    if (up.err) return up.err;
    for (int i = 0; i < F; ++i) fixed[i] = g->cam_fixed ? (g->cam_fixed[i] ? 1 : 0) : 1;
    d.n_free_cams = free_camera_slots(F, fixed, N, bb.cam, bb_ranges, e3.cam, e3_ranges, g->n_odom, g->odom_i, g->odom_j, extra_touched, slot);
    c->h_cam_slot.assign(slot, slot + F);
    c->h_od_i.assign(g->odom_i, g->odom_i + no); c->h_od_j.assign(g->odom_j, g->odom_j + no);
    std::copy(g->odom_i, g->odom_i + no, od_i);
    std::copy(g->odom_j, g->odom_j + no, od_j);
    std::copy(g->odom_meas, g->odom_meas + no * 7, od_meas);
    if (g->odom_info) std::copy(g->odom_info, g->odom_info + no * 6, od_info);
    else std::fill(od_info, od_info + no * 6, 1.0);
    odometry_csr(F, g->n_odom, g->odom_i, g->odom_j, cs, cp, pos);
  }
  mark();   // 6: cameras + odometry
  if ((rc = up.commit())) return rc;
  if ((rc = work_buffers(c, (size_t)N, (size_t)F, (size_t)c->n_chunks))) return rc;   // states + mapping-mode system
  if (d.n_free_cams == 0 && c->arena_solve.cap + c->arena_S.cap + c->arena_slam.cap > ((size_t)64 << 20)) {
    // a mapping-mode graph follows a SLAM-mode one: the solver blobs of the old graph (tens of GB at BASELINE configs[3]) would stay
    // pinned for the life of the context
    slam_trim(c, false);
  }
  if (d.n_free_cams > 0) {
    if ((rc = slam_alloc(c))) return rc;
  }
  mark();   // 7: commit + work arena + slam_alloc
  ESL_HIP_TRY(hipStreamSynchronize(st));
  mark();   // 8: copies landed
  if (host_timing) {
    std::fprintf(stderr, "esl_graph_upload us:");
    for (int i = 1; i < nht; ++i) std::fprintf(stderr, " %.0f", ht[i] - ht[i - 1]);
    std::fprintf(stderr, "  (validate, sort, gather, camera lists, chunks, cameras, commit, wait)\n");
  }
  c->graph_loaded = true;
  return ESL_OK;
}

extern "C" {

int esl_graph_upload(esl_ctx* c, const esl_graph* g) {
  if (!c) return ESL_ERR_INVALID;
  const int rc = validate_graph(g);
  if (rc) return rc;
  fx_clear(c);
  return graph_upload_impl(c, g, nullptr);
}

// ---------------------------------------------------------------------------------------------------
// esl_graph_upload_fixed: g2o's setFixed on ellipsoid vertices.  The caller's edges are split on the host: edges of free
// ellipsoids form an ordinary graph (same ellipsoid numbering; a fixed ellipsoid is an ellipsoid without edges, its state is
// copied through by every kernel that writes trial states), anchored edges (fixed ellipsoid, free camera) and inactive edges
// (fixed ellipsoid, fixed camera; every gravity prior of a fixed ellipsoid) go into the arrays of esl_fixed.hpp.
// ---------------------------------------------------------------------------------------------------
int esl_graph_upload_fixed(esl_ctx* c, const esl_graph* g, const uint8_t* obj_fixed) {
  if (!c) return ESL_ERR_INVALID;
  int rc = validate_graph(g);
  if (rc) return rc;
  bool any = false;
  if (obj_fixed) for (int o = 0; o < g->n_objs; ++o) any = any || obj_fixed[o] != 0;
  if (!any) { fx_clear(c); return graph_upload_impl(c, g, nullptr); }
  if (c->comm) { set_error("esl_graph_upload_fixed: fixed ellipsoids are not supported on a context with a communicator"); return ESL_ERR_STATE; }
  ESL_HIP_TRY(hipSetDevice(c->device));
  const int N = g->n_objs, F = g->n_cams;
  std::vector<uint8_t> fixed((size_t)N);
  for (int o = 0; o < N; ++o) fixed[o] = obj_fixed[o] ? 1 : 0;
  // One edge class of the caller's graph, split: (a) the edges of the free ellipsoids, caller order kept -- map[i] = their index
  // there --, (b) anchored and (c) inactive edges by caller index.  The arrays hold (a) for the upload, then (b) + (c) for the blob.
  struct Split { std::vector<int32_t> cam, obj; std::vector<double> meas, w; std::vector<int> map, anch, inact, start; };
  std::vector<uint8_t> touched((size_t)F, 0);
  auto edge_set = [](Split& s, size_t n, int width) { s.cam.resize(n); s.obj.resize(n); s.meas.resize(n * width); s.w.resize(n); return EdgeSet{s.cam.data(), s.obj.data(), s.meas.data(), s.w.data(), width}; };
  auto split = [&](const EdgeView& e, int n, Split& s) {
    size_t n_free = 0;
    s.map.resize((size_t)n);
    for (int i = 0; i < n; ++i) {
      if (!fixed[e.obj[i]]) s.map[i] = (int)n_free++;
      else if (g->cam_fixed && !g->cam_fixed[e.cam[i]]) { s.anch.push_back(i); touched[e.cam[i]] = 1; }
      else s.inact.push_back(i);
    }
    const EdgeSet dst = edge_set(s, n_free, e.width);
    for (int i = 0; i < n; ++i) if (!fixed[e.obj[i]]) copy_edge(dst, (size_t)s.map[i], e, (size_t)i);
    return (EdgeView)dst;
  };
  Split B, E;
  std::vector<int32_t> s_go;
  const EdgeView src_bb = bbox_edges(g), src_e3 = e3d_edges(g), sub_bb = split(src_bb, g->n_bbox, B), sub_e3 = split(src_e3, g->n_e3d, E);
  for (int i = 0; i < g->n_grav; ++i) if (!fixed[g->grav_obj[i]]) s_go.push_back(g->grav_obj[i]);
  esl_graph sub = *g;
  sub.n_bbox = (int32_t)B.cam.size(); sub.bbox_cam = sub_bb.cam; sub.bbox_obj = sub_bb.obj; sub.bbox_meas = sub_bb.meas; sub.bbox_weight = sub_bb.w;
  sub.n_e3d = (int32_t)E.cam.size(); sub.e3d_cam = sub_e3.cam; sub.e3d_obj = sub_e3.obj; sub.e3d_meas = sub_e3.meas; sub.e3d_weight = sub_e3.w;
  sub.n_grav = (int32_t)s_go.size(); sub.grav_obj = s_go.data();
  fx_clear(c);
  if ((rc = graph_upload_impl(c, &sub, touched.data()))) return rc;   // (returns with the stream synchronised: the staging block is free)
  // (b) sorted by camera (= by camera slot: slots ascend with the camera index), stable; (c) behind them; start = the anchored
  // edges of every camera slot
  const int nf = c->g.n_free_cams;
  auto anchor = [&](const EdgeView& e, Split& s) {
    std::stable_sort(s.anch.begin(), s.anch.end(), [&](int x, int y) { return e.cam[x] < e.cam[y]; });
    const size_t na = s.anch.size(), n = na + s.inact.size();
    const EdgeSet dst = edge_set(s, n, e.width);
    s.start.assign((size_t)nf + 1, 0);
    for (size_t k = 0; k < n; ++k) {
      const int i = k < na ? s.anch[k] : s.inact[k - na];
      copy_edge(dst, k, e, (size_t)i);
      s.map[i] = -((int)k + 1);
      if (k < na) ++s.start[(size_t)c->h_cam_slot[e.cam[i]] + 1];
    }
    for (int sl = 0; sl < nf; ++sl) s.start[(size_t)sl + 1] += s.start[sl];
  };
  anchor(src_bb, B); anchor(src_e3, E);
  // one blob: index arrays, measurements, flags, the per-slot lists, then -- device only -- the records
  AnchGraph& a = c->fx;
  const size_t nb = B.cam.size(), ne = E.cam.size(), n_rec = B.anch.size() + E.anch.size();
  const std::vector<unsigned char> valid(nb, 1);
  UploadStage st(c, &c->fx_blob, &c->fx_blob_cap);
  st.add(&a.bb_cam, B.cam.data(), nb); st.add(&a.bb_obj, B.obj.data(), nb); st.add(&a.bb_meas, B.meas.data(), nb * 4); st.add(&a.bb_w, B.w.data(), nb);
  st.add(&a.bb_valid, valid.data(), nb);
  st.add(&a.e3_cam, E.cam.data(), ne); st.add(&a.e3_obj, E.obj.data(), ne); st.add(&a.e3_meas, E.meas.data(), ne * 10); st.add(&a.e3_w, E.w.data(), ne);
  st.add(&a.bb_start, B.start.data(), B.start.size()); st.add(&a.e3_start, E.start.data(), E.start.size());
  if (st.err) return st.err;
  const size_t o_A = align_up(st.used, 256), o_chi = align_up(o_A + std::max<size_t>(n_rec * kARec * sizeof(double), 8), 256),
               total = align_up(o_chi + std::max<size_t>(n_rec * sizeof(double), 8), 256);
  if (total > c->fx_blob_cap) {   // (its own growth rule; with room made here, commit() below only copies)
    if (c->fx_blob) { (void)hipFree(c->fx_blob); c->fx_blob = nullptr; c->fx_blob_cap = 0; }
    ESL_HIP_TRY(hipMalloc((void**)&c->fx_blob, total + total / 8));
    c->fx_blob_cap = total + total / 8;
  }
  if ((rc = st.commit())) return rc;
  ESL_HIP_TRY(hipStreamSynchronize(c->stream));
  a.n_bb = (int)B.anch.size(); a.n_e3 = (int)E.anch.size(); a.n_bb_all = (int)nb; a.n_e3_all = (int)ne;
  c->fx_A = (double*)(c->fx_blob + o_A); c->fx_chi = (double*)(c->fx_blob + o_chi);
  c->fx_flags = fixed;
  c->fx_bb_map = B.map; c->fx_e3_map = E.map;
  c->fx_grav_obj.assign(g->grav_obj, g->grav_obj + g->n_grav);
  c->fx_on = true;
  return ESL_OK;
}

int esl_graph_obj_fixed(esl_ctx* c, uint8_t* flags_out, int32_t count) {
  if (!c || !flags_out) return ESL_ERR_INVALID;
  if (!c->graph_loaded) { set_error("esl_graph_obj_fixed: no graph loaded"); return ESL_ERR_STATE; }
  if (count != c->g.n_objs) { set_error("esl_graph_obj_fixed: count is not the graph's ellipsoid count"); return ESL_ERR_INVALID; }
  for (int o = 0; o < count; ++o) flags_out[o] = c->fx_on ? c->fx_flags[(size_t)o] : 0;
  return ESL_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------
// esl_graph_append: the appendable layout
// ---------------------------------------------------------------------------------------------------
// the image of the graph that is resident now (compact layout of esl_graph_upload), read back from the device
static int image_from_device(esl_ctx* c, HostImage& im) {
  const DevGraph& g = c->g;
  const int N = g.n_objs;
  im = HostImage();
  im.n_cams = g.n_cams; im.n_objs = N; im.n_grav = c->n_grav_edges;
  std::vector<int> bs((size_t)N + 1), es((size_t)N + 1);
  im.gr_cnt.assign((size_t)N, 0);
  im.bb.resize((size_t)g.n_bbox); im.e3.resize((size_t)g.n_e3d);
  im.cam_fixed.assign((size_t)g.n_cams, 1);
  im.od_i.resize((size_t)g.n_odom); im.od_j.resize((size_t)g.n_odom); im.od_meas.resize((size_t)g.n_odom * 7); im.od_info.resize((size_t)g.n_odom * 6);
  auto dl = [&](auto& dst, const void* src) -> int {
    if (!dst.empty()) ESL_HIP_TRY(hipMemcpyAsync(dst.data(), src, dst.size() * sizeof(dst[0]), hipMemcpyDeviceToHost, c->stream));
    return ESL_OK;
  };
  int rc;
  if ((rc = dl(bs, g.bb_start)) || (rc = dl(es, g.e3_start)) || (rc = dl(im.gr_cnt, g.gr_cnt)) ||
      (rc = dl(im.bb.cam, g.bb_cam)) || (rc = dl(im.bb.obj, g.bb_obj)) || (rc = dl(im.bb.meas, g.bb_meas)) || (rc = dl(im.bb.w, g.bb_w)) ||
      (rc = dl(im.e3.cam, g.e3_cam)) || (rc = dl(im.e3.obj, g.e3_obj)) || (rc = dl(im.e3.meas, g.e3_meas)) || (rc = dl(im.e3.w, g.e3_w)) ||
      (rc = dl(im.cam_fixed, g.cam_fixed)) || (rc = dl(im.od_i, g.od_i)) || (rc = dl(im.od_j, g.od_j)) || (rc = dl(im.od_meas, g.od_meas)) ||
      (rc = dl(im.od_info, g.od_info)))
    return rc;
  ESL_HIP_TRY(hipStreamSynchronize(c->stream));
  auto compact = [&](EdgeSlices& s, const std::vector<int>& start, int n) {   // every slice exactly full
    s.begin.assign(start.begin(), start.end() - 1);
    s.cnt.resize((size_t)N);
    for (int o = 0; o < N; ++o) s.cnt[o] = start[(size_t)o + 1] - start[o];
    s.slice_cap = s.cnt;
    s.used = s.cap = (size_t)n;
  };
  compact(im.bb, bs, g.n_bbox); compact(im.e3, es, g.n_e3d);
  im.cap_cams = im.n_cams; im.cap_objs = N;
  return ESL_OK;
}

// a fresh image with slack: every slice doubled (+ 64 / 32), arrays and vertex counts with room for as much again
static void image_relayout(const HostImage& old, HostImage& im, const std::vector<int>& add_bb, const std::vector<int>& add_e3, int n_cams, int n_objs) {
  im = HostImage();
  im.appendable = true;
  im.relayouts = old.relayouts + 1;
  im.n_cams = n_cams; im.n_objs = n_objs; im.n_grav = old.n_grav;
  im.cam_fixed = old.cam_fixed; im.od_i = old.od_i; im.od_j = old.od_j; im.od_meas = old.od_meas; im.od_info = old.od_info;
  im.cap_cams = n_cams * 2 + 64; im.cap_objs = n_objs * 2 + 16;
  im.gr_cnt.assign((size_t)n_objs, 0);
  std::copy(old.gr_cnt.begin(), old.gr_cnt.begin() + old.n_objs, im.gr_cnt.begin());
  auto relay = [&](const EdgeSlices& from, EdgeSlices& s, const std::vector<int>& add, size_t chunk) {
    s.begin.resize((size_t)n_objs); s.cnt.assign((size_t)n_objs, 0); s.slice_cap.resize((size_t)n_objs);
    size_t p = 0;
    for (int o = 0; o < n_objs; ++o) {
      s.begin[o] = (int)p; s.slice_cap[o] = (int)s.slice_capacity((size_t)((o < old.n_objs ? from.cnt[o] : 0) + add[o])); p += (size_t)s.slice_cap[o];
    }
    s.used = p;
    s.cap = p + p / 2 + chunk * 64;   // room for ellipsoids that do not exist yet
    s.cam.assign(s.cap, 0); s.obj.assign(s.cap, -1); s.meas.assign(s.cap * s.width, 0.0); s.w.assign(s.cap, 0.0);
    for (int o = 0; o < old.n_objs; ++o) {
      for (int k = 0; k < from.cnt[o]; ++k) copy_edge(s.set(), (size_t)s.begin[o] + k, from.view(), (size_t)from.begin[o] + k);
      s.cnt[o] = from.cnt[o];
    }
  };
  relay(old.bb, im.bb, add_bb, 64); relay(old.e3, im.e3, add_e3, 32);
}

// SLAM mode of the appendable layout: everything that is indexed by CAMERA -- fixed flags, free-camera slots, the per-camera lists
// of bbox / 3-D / odometry edges -- and the odometry arrays are rebuilt from the host image by the rules esl_graph_upload uses and
// shipped as ONE blob into a grow-only buffer of their own (a few bytes per edge: 2 MB at BASELINE configs[3], nothing at streaming
// sizes); then the solver-side lists of esl_slam.hip (slam_alloc) are rebuilt from the same mirror.  The edge records and the
// states stay where they are.  The caller has synchronised the stream: the staging block is free.
static int slam_tables_refresh(esl_ctx* c, const HostImage& im) {
  DevGraph& d = c->g;
  const int F = im.n_cams, N = im.n_objs, no = (int)im.od_i.size();
  const size_t nb = (size_t)im.bb.n_edges(), ne = (size_t)im.e3.n_edges();
  std::vector<unsigned char> fixed((size_t)F, 1);
  for (int i = 0; i < F && i < (int)im.cam_fixed.size(); ++i) fixed[i] = im.cam_fixed[i] ? 1 : 0;
  std::vector<int> slot((size_t)F), pos;
  std::vector<int> cbs((size_t)F + 1), cbe(std::max<size_t>(nb, 1)), ces((size_t)F + 1), cee(std::max<size_t>(ne, 1)), cos((size_t)F + 1), coe((size_t)no * 2);
  const int nf = free_camera_slots(F, fixed.data(), N, im.bb.cam.data(), im.bb.ranges(), im.e3.cam.data(), im.e3.ranges(), no, im.od_i.data(), im.od_j.data(),
                                   nullptr, slot.data());
  camera_csr(F, N, im.bb.cam.data(), im.bb.ranges(), cbs.data(), cbe.data(), pos);
  camera_csr(F, N, im.e3.cam.data(), im.e3.ranges(), ces.data(), cee.data(), pos);
  odometry_csr(F, no, im.od_i.data(), im.od_j.data(), cos.data(), coe.data(), pos);
  UploadStage st(c, &c->slam_tab_dev, &c->slam_tab_cap);
  st.add(&d.cam_fixed, fixed.data(), (size_t)F); st.add(&d.cam_slot, slot.data(), (size_t)F);
  st.add(&d.cbb_start, cbs.data(), cbs.size()); st.add(&d.cbb_edge, cbe.data(), nb);
  st.add(&d.ce3_start, ces.data(), ces.size()); st.add(&d.ce3_edge, cee.data(), ne);
  st.add(&d.cod_start, cos.data(), cos.size()); st.add(&d.cod_edge, coe.data(), coe.size());
  st.add(&d.od_i, im.od_i.data(), (size_t)no); st.add(&d.od_j, im.od_j.data(), (size_t)no);
  st.add(&d.od_meas, im.od_meas.data(), (size_t)no * 7); st.add(&d.od_info, im.od_info.data(), (size_t)no * 6);
  int rc = st.commit();
  if (rc) return rc;
  d.n_free_cams = nf; d.n_odom = no;
  // the mirrors slam_alloc reads: position-indexed, free slots carry obj = -1
  c->h_cam_slot = slot;
  c->h_od_i = im.od_i; c->h_od_j = im.od_j;
  c->h_bb_cam.assign(im.bb.cam.begin(), im.bb.cam.begin() + (long)im.bb.used); c->h_bb_obj.assign(im.bb.obj.begin(), im.bb.obj.begin() + (long)im.bb.used);
  c->h_e3_cam.assign(im.e3.cam.begin(), im.e3.cam.begin() + (long)im.e3.used); c->h_e3_obj.assign(im.e3.obj.begin(), im.e3.obj.begin() + (long)im.e3.used);
  slam_forget(c);
  ESL_HIP_TRY(hipStreamSynchronize(c->stream));   // the staging block is free again (slam_alloc stages through its own blob)
  if (nf > 0 && (rc = slam_alloc(c))) return rc;
  return ESL_OK;
}

// the whole image to the device (capacities included) + the states; replaces what esl_graph_upload laid out
static int image_upload(esl_ctx* c, const HostImage& im, const double* cams, const double* objs, const DevGraph& settings) {
  free_graph(c);
  DevGraph& d = c->g;
  UploadStage up(c, &c->arena_graph, &c->arena_graph_cap);
  d = DevGraph();
  d.n_cams = im.n_cams; d.n_objs = im.n_objs; d.n_bbox = (int)im.bb.used; d.n_e3d = (int)im.e3.used; d.n_odom = 0;
  d.n_bbox_edges = im.bb.n_edges();
  for (int k = 0; k < 4; ++k) d.K[k] = settings.K[k];
  for (int k = 0; k < 3; ++k) d.grav_n[k] = settings.grav_n[k];
  d.grav_w = settings.grav_w; d.yt = settings.yt; d.check_vis = settings.check_vis; d.img_rows = settings.img_rows; d.img_cols = settings.img_cols;
  const size_t cN = (size_t)im.cap_objs, cF = (size_t)im.cap_cams;
  std::vector<int> gr(cN, 0);
  std::copy(im.gr_cnt.begin(), im.gr_cnt.begin() + im.n_objs, gr.begin());
  std::vector<unsigned char> valid(im.bb.cap, 0);   // slack slots stay invalid; an append marks the slots it fills
  for (int o = 0; o < im.n_objs; ++o) std::fill_n(valid.begin() + im.bb.begin[o], im.bb.cnt[o], 1);
  const std::vector<int> bbs = im.bb.starts(cN + 1), e3s = im.e3.starts(cN + 1);
  up.add(&d.bb_start, bbs.data(), bbs.size());
  up.add(&d.e3_start, e3s.data(), e3s.size());
  up.add(&d.gr_cnt, gr.data(), gr.size());
  up.add(&d.bb_cam, im.bb.cam.data(), im.bb.cap); up.add(&d.bb_obj, im.bb.obj.data(), im.bb.cap);
  up.add(&d.bb_meas, im.bb.meas.data(), im.bb.cap * 4); up.add(&d.bb_w, im.bb.w.data(), im.bb.cap);
  up.add(&d.bb_valid, valid.data(), valid.size());
  up.add(&d.e3_cam, im.e3.cam.data(), im.e3.cap); up.add(&d.e3_obj, im.e3.obj.data(), im.e3.cap);
  up.add(&d.e3_meas, im.e3.meas.data(), im.e3.cap * 10); up.add(&d.e3_w, im.e3.w.data(), im.e3.cap);
  // the chunk table, zero-padded to the capacity of the arrays
  const size_t cap_chunks = chunk_capacity(im.bb.cap, im.e3.cap, cN);
  std::vector<int> tab(Chunks::ints(cap_chunks, cN), 0);
  Chunks t = Chunks::in(tab.data(), cap_chunks);
  build_chunks(im.n_objs, im.bb.ranges(), im.e3.ranges(), t);
  c->n_chunks = t.n_chunks; c->n_ids_bb = t.n_ids_bb; c->n_ids_e3 = t.n_ids_e3;
  up.add(&c->ck_obj, t.obj, cap_chunks); up.add(&c->ck_type, t.type, cap_chunks); up.add(&c->ck_begin, t.begin, cap_chunks);
  up.add(&c->ck_end, t.end, cap_chunks); up.add(&c->ck_ostart, t.ostart, cN + 1);
  up.add(&c->ck_ids_bb, t.ids_bb, cap_chunks); up.add(&c->ck_ids_e3, t.ids_e3, cap_chunks);
  // mapping-mode camera tables (slam_tables_refresh replaces them when the image has free cameras or odometry)
  std::vector<unsigned char> fixed(cF, 1);
  std::vector<int> slot(cF, -1), one(2, 0);
  up.add(&d.cam_fixed, fixed.data(), fixed.size());
  up.add(&d.cam_slot, slot.data(), slot.size());
  d.n_free_cams = 0;
  c->h_cam_slot.assign(cF, -1); c->h_bb_cam.clear(); c->h_bb_obj.clear(); c->h_e3_cam.clear(); c->h_e3_obj.clear();
  const double dz[8] = {0};
  up.add(&d.od_i, one.data(), 1); up.add(&d.od_j, one.data(), 1); up.add(&d.od_meas, dz, 7); up.add(&d.od_info, dz, 6);
  up.add(&d.cbb_start, one.data(), 2); up.add(&d.cbb_edge, one.data(), 1); up.add(&d.ce3_start, one.data(), 2); up.add(&d.ce3_edge, one.data(), 1);
  up.add(&d.cod_start, one.data(), 2); up.add(&d.cod_edge, one.data(), 1);
  int rc;
  if ((rc = up.commit())) return rc;
  if ((rc = work_buffers(c, cN, cF, cap_chunks))) return rc;
  if (im.n_cams) ESL_HIP_TRY(hipMemcpyAsync(c->cams, cams, (size_t)im.n_cams * 7 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if (im.n_objs) ESL_HIP_TRY(hipMemcpyAsync(c->objs, objs, (size_t)im.n_objs * 10 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  ESL_HIP_TRY(hipStreamSynchronize(c->stream));
  c->n_grav_edges = im.n_grav;
  c->graph_loaded = true; c->states_loaded = true; c->cams_match_snap = false; c->lm.begun = false;
  if (im.slam()) return slam_tables_refresh(c, im);
  return ESL_OK;
}

// a new edge as the record k_append_scatter places (AppendBb / AppendE3)
template <class Rec>
static void push_record(std::vector<Rec>& out, int slot, const EdgeView& e, size_t i) {
  Rec r{};
  r.slot = slot; r.cam = e.cam[i]; r.obj = e.obj[i]; r.w = e.w[i];
  std::memcpy(r.meas, e.meas + i * e.width, sizeof(r.meas));
  out.push_back(r);
}

extern "C" {

int esl_graph_sizes(esl_ctx* c, int32_t* n_cams, int32_t* n_objs, int32_t* n_bbox, int32_t* n_e3d, int32_t* relayouts) {
  if (!c || !c->graph_loaded) return ESL_ERR_STATE;
  const HostImage* im = c->append_img;
  if (n_cams) *n_cams = c->g.n_cams;
  if (n_objs) *n_objs = c->g.n_objs;
  if (n_bbox) *n_bbox = c->g.n_bbox_edges;
  if (n_e3d) *n_e3d = im ? im->e3.n_edges() : c->g.n_e3d;
  if (relayouts) *relayouts = im ? im->relayouts : 0;
  return ESL_OK;
}

int esl_graph_append(esl_ctx* c, const esl_graph_delta* dl) {
  if (c && c->fx_on) { set_error("esl_graph_append: the resident graph has fixed ellipsoids (esl_graph_upload_fixed); upload the extended graph instead"); return ESL_ERR_STATE; }
  if (!c || !dl) return ESL_ERR_INVALID;
  if (!c->graph_loaded || !c->states_loaded) { set_error("esl_graph_append: upload a graph and its states first"); return ESL_ERR_STATE; }
  if (c->comm) { set_error("esl_graph_append: one GPU only (no communicator)"); return ESL_ERR_STATE; }
  if (dl->n_odom < 0 || (dl->n_odom && (!dl->odom_i || !dl->odom_j || !dl->odom_meas))) { set_error("esl_graph_delta: null odometry array or negative size"); return ESL_ERR_INVALID; }
  if (dl->n_new_cams < 0 || dl->n_new_objs < 0 || dl->n_bbox < 0 || dl->n_e3d < 0 || dl->n_grav < 0 || (dl->n_new_cams && !dl->new_cams) ||
      (dl->n_new_objs && !dl->new_objs) || (dl->n_bbox && (!dl->bbox_cam || !dl->bbox_obj || !dl->bbox_meas || !dl->bbox_weight)) ||
      (dl->n_e3d && (!dl->e3d_cam || !dl->e3d_obj || !dl->e3d_meas || !dl->e3d_weight)) || (dl->n_grav && !dl->grav_obj)) {
    set_error("esl_graph_delta: null array or negative size"); return ESL_ERR_INVALID;
  }
  ESL_HIP_TRY(hipSetDevice(c->device));
  int rc;
  if (!c->append_img) {
    HostImage* im0 = new HostImage();
    if ((rc = image_from_device(c, *im0))) { delete im0; return rc; }
    c->append_img = im0;
  }
  HostImage& im = *c->append_img;
  const int F = im.n_cams + dl->n_new_cams, N = im.n_objs + dl->n_new_objs;
  const EdgeView new_bb{dl->bbox_cam, dl->bbox_obj, dl->bbox_meas, dl->bbox_weight, 4}, new_e3{dl->e3d_cam, dl->e3d_obj, dl->e3d_meas, dl->e3d_weight, 10};
  if ((rc = check_indices("esl_graph_delta", F, N, new_bb, dl->n_bbox, new_e3, dl->n_e3d, dl->grav_obj, dl->n_grav, dl->odom_i, dl->odom_j, dl->n_odom))) return rc;
  c->graph_fp += fp_edges(1, dl->n_bbox, dl->bbox_cam, dl->bbox_obj) + fp_edges(2, dl->n_e3d, dl->e3d_cam, dl->e3d_obj) + fp_edges(3, dl->n_odom, dl->odom_i, dl->odom_j) +
                 fp_fixed(im.n_cams, dl->n_new_cams, dl->new_cam_fixed);
  c->repl_checked = false;
  auto add_cameras_and_odometry = [&](HostImage& I) {   // the delta's camera flags and odometry edges into an image whose n_cams is already F
    I.cam_fixed.resize((size_t)F, 1);
    for (int i = 0; i < dl->n_new_cams; ++i) I.cam_fixed[(size_t)(F - dl->n_new_cams + i)] = dl->new_cam_fixed ? (dl->new_cam_fixed[i] ? 1 : 0) : 1;
    for (int i = 0; i < dl->n_odom; ++i) {
      I.od_i.push_back(dl->odom_i[i]); I.od_j.push_back(dl->odom_j[i]);
      for (int q = 0; q < 7; ++q) I.od_meas.push_back(dl->odom_meas[(size_t)i * 7 + q]);
      for (int q = 0; q < 6; ++q) I.od_info.push_back(dl->odom_info ? dl->odom_info[(size_t)i * 6 + q] : 1.0);
    }
  };
  std::vector<int> add_bb((size_t)N, 0), add_e3((size_t)N, 0), add_gr((size_t)N, 0);
  for (int i = 0; i < dl->n_bbox; ++i) add_bb[dl->bbox_obj[i]]++;
  for (int i = 0; i < dl->n_e3d; ++i) add_e3[dl->e3d_obj[i]]++;
  for (int i = 0; i < dl->n_grav; ++i) add_gr[dl->grav_obj[i]]++;
  for (int o = 0; o < N; ++o)
    if ((o < im.n_objs ? im.gr_cnt[o] : 0) + add_gr[o] > 64) { set_error("more than 64 gravity edges on one ellipsoid"); return ESL_ERR_INVALID; }
  // does everything fit the slack of the resident layout?  (new ellipsoids get their slices at the end of the arrays)
  auto fits_slack = [&](const EdgeSlices& s, const std::vector<int>& add) {
    size_t end = s.used;
    for (int o = 0; o < im.n_objs; ++o) if (s.cnt[o] + add[o] > s.slice_cap[o]) return false;
    for (int o = im.n_objs; o < N; ++o) end += s.slice_capacity((size_t)add[o]);
    return end <= s.cap;
  };
  const bool fits = im.appendable && F <= im.cap_cams && N <= im.cap_objs && fits_slack(im.bb, add_bb) && fits_slack(im.e3, add_e3);
  std::vector<AppendBb> rb;
  std::vector<AppendE3> re;
  // the new edges into the free slots of I (arrival order inside an ellipsoid); records: what the incremental path ships
  auto place_edges = [&](EdgeSlices& s, const EdgeView& e, int n, std::vector<int>& slot_of, auto* records) {
    for (int i = 0; i < n; ++i) {
      const int o = e.obj[i];
      const size_t at = (size_t)s.begin[o] + s.cnt[o]++;
      copy_edge(s.set(), at, e, (size_t)i);
      slot_of.push_back((int)at);
      if (records) push_record(*records, (int)at, e, (size_t)i);
    }
  };
  auto place = [&](HostImage& I, bool record) {
    place_edges(I.bb, new_bb, dl->n_bbox, c->h_bb_slot_of, record ? &rb : nullptr);
    place_edges(I.e3, new_e3, dl->n_e3d, c->h_e3_slot_of, record ? &re : nullptr);
    for (int o = 0; o < N; ++o) I.gr_cnt[o] += add_gr[o];
    I.n_grav += dl->n_grav;
    c->h_grav_obj.insert(c->h_grav_obj.end(), dl->grav_obj, dl->grav_obj + dl->n_grav);
  };
  if (!fits) {
    // full re-layout with doubled slack: the states that live on the device come back first
    std::vector<double> cams((size_t)F * 7), objs((size_t)N * 10);
    if (im.n_cams) ESL_HIP_TRY(hipMemcpyAsync(cams.data(), c->cams, (size_t)im.n_cams * 7 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (im.n_objs) ESL_HIP_TRY(hipMemcpyAsync(objs.data(), c->objs, (size_t)im.n_objs * 10 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    ESL_HIP_TRY(hipStreamSynchronize(c->stream));
    for (size_t k = 0; k < (size_t)dl->n_new_cams * 7; ++k) cams[(size_t)im.n_cams * 7 + k] = dl->new_cams[k];
    for (size_t k = 0; k < (size_t)dl->n_new_objs * 10; ++k) objs[(size_t)im.n_objs * 10 + k] = dl->new_objs[k];
    HostImage* ni = new HostImage();
    image_relayout(im, *ni, add_bb, add_e3, F, N);
    // the caller's edges move with their ellipsoid's slice (same position inside it)
    auto moved = [](std::vector<int>& slot_of, const EdgeSlices& from, const EdgeSlices& to) {
      for (int& sl : slot_of) { const int o = from.obj[sl]; sl = to.begin[o] + (sl - from.begin[o]); }
    };
    moved(c->h_bb_slot_of, im.bb, ni->bb); moved(c->h_e3_slot_of, im.e3, ni->e3);
    place(*ni, false);
    add_cameras_and_odometry(*ni);
    const DevGraph gd = c->g;   // K, gravity, yaw table, visibility settings survive a re-layout
    c->append_img = nullptr;   // free_graph (inside image_upload) must not drop the image under construction
    rc = image_upload(c, *ni, cams.data(), objs.data(), gd);
    delete &im;
    if (rc) { delete ni; return rc; }
    c->append_img = ni;
    dev_free(&c->cams_snap); dev_free(&c->objs_snap);
    return ESL_OK;
  }
  // incremental: slices of the new ellipsoids at the end of the arrays, edges into free slots, tables rebuilt on the host
  auto new_slices = [&](EdgeSlices& s, const std::vector<int>& add) {
    s.begin.resize((size_t)N); s.cnt.resize((size_t)N, 0); s.slice_cap.resize((size_t)N);
    for (int o = im.n_objs; o < N; ++o) { s.begin[o] = (int)s.used; s.slice_cap[o] = (int)s.slice_capacity((size_t)add[o]); s.used += (size_t)s.slice_cap[o]; }
  };
  new_slices(im.bb, add_bb); new_slices(im.e3, add_e3);
  im.gr_cnt.resize((size_t)N, 0);
  const int F0 = im.n_cams, N0 = im.n_objs;
  im.n_cams = F; im.n_objs = N;
  place(im, true);
  add_cameras_and_odometry(im);
  const size_t cap_chunks = chunk_capacity(im.bb.used, im.e3.used, (size_t)N);
  std::vector<int> tab(Chunks::ints(cap_chunks, (size_t)N));
  Chunks t = Chunks::in(tab.data(), cap_chunks);
  build_chunks(N, im.bb.ranges(), im.e3.ranges(), t);
  const std::vector<int> bbs = im.bb.starts((size_t)N + 1), e3s = im.e3.starts((size_t)N + 1);   // with the end sentinel, as in image_upload
  // one staged blob: tables | bbox records | 3-D records; k_append_tables / k_append_scatter move them to their places
  DevGraph& g = c->g;
  UploadStage st(c, &c->append_dev, &c->append_dev_cap);
  AppendCopies cp{};
  int* staged[12];
  auto tab_copy = [&](const int* src, size_t n, int* dst) { st.add(&staged[cp.n], src, n); cp.dst[cp.n] = dst; cp.count[cp.n] = (int)n; ++cp.n; };
  tab_copy(t.obj, (size_t)t.n_chunks, c->ck_obj); tab_copy(t.type, (size_t)t.n_chunks, c->ck_type); tab_copy(t.begin, (size_t)t.n_chunks, c->ck_begin);
  tab_copy(t.end, (size_t)t.n_chunks, c->ck_end); tab_copy(t.ostart, (size_t)N + 1, c->ck_ostart); tab_copy(t.ids_bb, (size_t)t.n_ids_bb, c->ck_ids_bb);
  tab_copy(t.ids_e3, (size_t)t.n_ids_e3, c->ck_ids_e3); tab_copy(im.gr_cnt.data(), im.gr_cnt.size(), g.gr_cnt); tab_copy(bbs.data(), bbs.size(), g.bb_start);
  tab_copy(e3s.data(), e3s.size(), g.e3_start);
  AppendBb* d_rb = nullptr;
  AppendE3* d_re = nullptr;
  st.add(&d_rb, rb.data(), rb.size()); st.add(&d_re, re.data(), re.size());
  if ((rc = st.commit())) return rc;
  for (int k = 0; k < cp.n; ++k) cp.src[k] = staged[k];
  g.n_cams = F; g.n_objs = N; g.n_bbox = (int)im.bb.used; g.n_e3d = (int)im.e3.used; g.n_bbox_edges += dl->n_bbox;
  c->n_chunks = t.n_chunks; c->n_ids_bb = t.n_ids_bb; c->n_ids_e3 = t.n_ids_e3;
  c->n_grav_edges = im.n_grav;
  hipLaunchKernelGGL(k_append_tables, dim3(16), dim3(256), 0, c->stream, cp);
  const int n_rec = (int)(rb.size() + re.size());
  if (n_rec)
    hipLaunchKernelGGL(k_append_scatter, dim3((n_rec + 127) / 128), dim3(128), 0, c->stream, g, (const AppendBb*)d_rb, (int)rb.size(), (const AppendE3*)d_re, (int)re.size());
  ESL_HIP_TRY(hipGetLastError());
  if (dl->n_new_cams) ESL_HIP_TRY(hipMemcpyAsync(c->cams + (size_t)F0 * 7, dl->new_cams, (size_t)dl->n_new_cams * 7 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if (dl->n_new_objs) ESL_HIP_TRY(hipMemcpyAsync(c->objs + (size_t)N0 * 10, dl->new_objs, (size_t)dl->n_new_objs * 10 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  ESL_HIP_TRY(hipStreamSynchronize(c->stream));   // the caller's buffers and the staging block are free again
  dev_free(&c->cams_snap); dev_free(&c->objs_snap);
  c->cams_match_snap = false;
  c->lm.begun = false;
  if (im.slam()) {   // the camera-indexed tables + the solver's lists (SLAM mode)
    // Not failure-atomic by itself: records, states and the host image are committed above, the camera tables are rebuilt here.  If
    // that fails (out of memory in arena_reserve / slam_alloc) the device tables may be freed or describe the old graph -- drop the
    // graph altogether, so that the next call is an error ("upload graph first") and never a read of stale tables.
    const int rcs = slam_tables_refresh(c, im);
    if (rcs) { const std::string msg = esl_last_error(); free_graph(c); set_error(msg + " (esl_graph_append: the graph was dropped, upload it again)"); return rcs; }
  }
  return ESL_OK;
}

// ---------------------------------------------------------------------------------------------------
// states
// ---------------------------------------------------------------------------------------------------
int esl_states_upload(esl_ctx* c, const double* cams, const double* objs) {
  if (!c || !c->graph_loaded) { set_error("esl_states_upload: no graph loaded"); return ESL_ERR_STATE; }
  if ((c->g.n_cams && !cams) || (c->g.n_objs && !objs)) return ESL_ERR_INVALID;
  ESL_HIP_TRY(hipSetDevice(c->device));
  if (c->g.n_cams) ESL_HIP_TRY(hipMemcpyAsync(c->cams, cams, (size_t)c->g.n_cams * 7 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if (c->g.n_objs) ESL_HIP_TRY(hipMemcpyAsync(c->objs, objs, (size_t)c->g.n_objs * 10 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  ESL_HIP_TRY(hipStreamSynchronize(c->stream));
  c->states_loaded = true;
  c->cams_match_snap = false;
  c->lm.begun = false;
  return ESL_OK;
}

int esl_states_download(esl_ctx* c, double* cams, double* objs) {
  if (!c || !c->states_loaded) { set_error("esl_states_download: no states"); return ESL_ERR_STATE; }
  ESL_HIP_TRY(hipSetDevice(c->device));
  if (cams && c->g.n_cams) ESL_HIP_TRY(hipMemcpyAsync(cams, c->cams, (size_t)c->g.n_cams * 7 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (objs && c->g.n_objs) ESL_HIP_TRY(hipMemcpyAsync(objs, c->objs, (size_t)c->g.n_objs * 10 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  ESL_HIP_TRY(hipStreamSynchronize(c->stream));
  return ESL_OK;
}

int esl_states_snapshot(esl_ctx* c) {
  if (!c || !c->states_loaded) { set_error("esl_states_snapshot: no states"); return ESL_ERR_STATE; }
  ESL_HIP_TRY(hipSetDevice(c->device));
  const size_t nc = (size_t)c->g.n_cams * 7, no = (size_t)c->g.n_objs * 10;
  if (!c->cams_snap) ESL_HIP_TRY(hipMalloc((void**)&c->cams_snap, std::max<size_t>(nc, 1) * sizeof(double)));
  if (!c->objs_snap) ESL_HIP_TRY(hipMalloc((void**)&c->objs_snap, std::max<size_t>(no, 1) * sizeof(double)));
  if (nc) ESL_HIP_TRY(hipMemcpyAsync(c->cams_snap, c->cams, nc * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  if (no) ESL_HIP_TRY(hipMemcpyAsync(c->objs_snap, c->objs, no * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  c->cams_match_snap = true;
  return ESL_OK;
}

int esl_states_restore(esl_ctx* c) {
  if (!c || !c->cams_snap || !c->objs_snap) { set_error("esl_states_restore: no snapshot"); return ESL_ERR_STATE; }
  ESL_HIP_TRY(hipSetDevice(c->device));
  const size_t nc = (size_t)c->g.n_cams * 7, no = (size_t)c->g.n_objs * 10;
  if (nc && !c->cams_match_snap) ESL_HIP_TRY(hipMemcpyAsync(c->cams, c->cams_snap, nc * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  c->cams_match_snap = true;
  if (no) ESL_HIP_TRY(hipMemcpyAsync(c->objs, c->objs_snap, no * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  c->lm.begun = false;
  return ESL_OK;
}

}  // extern "C"
