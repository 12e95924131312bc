// esl_dense_int.hpp — what the seven units of the dense map share: esl_dense.hip (the map), esl_dense_objects.hip and
// esl_dense_planes.hip (the two extractors that read it), esl_dense_render.hip (the view of it), esl_dense_align.hip (its normals
// and the poses refined against it), esl_dense_carve.hip (the voxels that later frames see through) and esl_dense_covis.hip (the
// frames' covisibility through it).  The record and the counters,
// the map's state and its buffers, the probes of the voxel table, the sorted list of the live voxels as one step (DenseList,
// dense_list_begin / _launch: defined in esl_dense.hip, whose kernels they launch), the growth of a unit's own buffers from a table
// (DenseSlot, dense_grow) and the entries' small helpers (dense_fail, dense_begun, dense_map_invalid).  What an entry refuses for a
// parameter's value alone is esl_dense_check.hpp's.  Internal: only those seven units include it.
// The rule of all seven: every store to global memory is a vector store or an atomic in plain C++; no loop waits for another thread: a
// probe that finds no slot within the table's size, or a map over its capacity, raises the sticky status 3 and gives up.
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "esl_ctx.hpp"
#include "esl_dense_key.hpp"

namespace esl {

static_assert(sizeof(esl_dense_params) == 40, "include/esl.h states this size");
static_assert(sizeof(esl_dense_add_result) == 48, "include/esl.h states this size");
static_assert(sizeof(esl_dense_info) == 32, "include/esl.h states this size");
static_assert(sizeof(esl_dense_remove_result) == 64, "include/esl.h states this size");
static_assert(sizeof(esl_dense_move_result) == 120, "include/esl.h states this size");
static_assert(sizeof(esl_dense_slots) == 32, "include/esl.h states this size");
static_assert(sizeof(esl_dense_obj_params) == 32, "include/esl.h states this size");
static_assert(sizeof(esl_dense_obj_result) == 32, "include/esl.h states this size");
static_assert(sizeof(esl_dense_plane_params) == 80, "include/esl.h states this size");
static_assert(sizeof(esl_dense_plane_result) == 32, "include/esl.h states this size");
static_assert(sizeof(esl_dense_render_params) == 56, "include/esl.h states this size");
static_assert(sizeof(esl_dense_render_result) == 16, "include/esl.h states this size");
static_assert(sizeof(esl_dense_normal_params) == 24, "include/esl.h states this size");
static_assert(sizeof(esl_dense_normal_result) == 16, "include/esl.h states this size");
static_assert(sizeof(esl_dense_align_params) == 80, "include/esl.h states this size");
static_assert(sizeof(esl_dense_align_frame) == 384, "include/esl.h states this size");
static_assert(sizeof(esl_dense_align_result) == 16, "include/esl.h states this size");
static_assert(sizeof(esl_dense_carve_params) == 48, "include/esl.h states this size");
static_assert(sizeof(esl_dense_carve_result) == 96, "include/esl.h states this size");
static_assert(sizeof(esl_dense_covis_params) == 56, "include/esl.h states this size");
static_assert(sizeof(esl_dense_covis_result) == 32, "include/esl.h states this size");

constexpr int kDenseThreads = 256;
typedef unsigned long long u64;

struct DenseRec { long long S[3]; u64 col[3]; u64 count; u64 best; };
static_assert(sizeof(DenseRec) == 64, "one record per 64-byte segment");

// the device counters: this call's five counts, then what lives as long as the map
// (DC_VOXELS / DC_PAIRS count the slots CLAIMED since esl_dense_begin or the last purge), then a removing call's n_missing, the audit's
// five words and the purge's two list lengths
enum { DC_SAMPLED, DC_ZERO, DC_DEPTH_OUT, DC_KEY_OUT, DC_USED, DC_VOXELS, DC_PAIRS, DC_STATUS, DC_LIST,
       DC_MISSING, DC_LIVE_V, DC_DEAD_V, DC_LIVE_P, DC_DEAD_P, DC_BAD, DC_XV, DC_XP, DC_COUNT };

// the map's buffers: the tables, a call's uploads, the sorted list and esl_dense_extract's outputs, then esl_dense_move_frames' second
// pose set and esl_dense_purge's live records and pairs.  Each extractor keeps a set of its own, its slots named in its unit.
enum { DB_KEYS, DB_REC, DB_PKEYS, DB_PCNT, DB_CTR, DB_POSE, DB_DEPTH, DB_BGR, DB_INST, DB_LKEY, DB_LVAL, DB_SKEY, DB_SVAL, DB_TEMP,
       DB_OKEY, DB_OXYZ, DB_OCNT, DB_OBGR, DB_OINST, DB_OVOTES, DB_POSE2, DB_XKEY, DB_XREC, DB_XPKEY, DB_XPID, DB_XPCNT, DB_COUNT };
constexpr int kDobjBufs = 17, kDplBufs = 12, kDrnBufs = 14, kDalBufs = 11, kDcvBufs = 14, kDcoBufs = 12;   // the lengths of the other units' own enums (asserted there)
struct DenseState {
  ScratchSet<DB_COUNT> set;
  ScratchSet<kDobjBufs> obj_set;   // esl_dense_objects
  ScratchSet<kDplBufs> pl_set;     // esl_dense_planes
  ScratchSet<kDrnBufs> rn_set;     // esl_dense_render
  ScratchSet<kDalBufs> al_set;     // esl_dense_normals, esl_dense_align_frames
  ScratchSet<kDcvBufs> cv_set;     // esl_dense_carve_frames
  ScratchSet<kDcoBufs> co_set;     // esl_dense_covis_frames
  bool begun = false, combine = true;
  esl_dense_params p;
  int with_color = 0, with_inst = 0;
  u64 H = 0;
  long long n_samples = 0, n_voxels = 0, n_pairs = 0;   // n_voxels, n_pairs: LIVE slots (what k_dense_compact lists, what votes)
  long long dead_voxels = 0, dead_pairs = 0;             // claimed slots whose count is 0 (steps 9 to 11); claimed = live + dead
  int status = 0;
  std::vector<double> cams, pose, cams2, pose2;   // host staging of a call's poses (esl_dense_move_frames: both sets)
  std::vector<int> moved;                         // esl_dense_move_frames: the frames whose pose changed
  std::vector<uint16_t> carved_depth;             // esl_dense_carve_frames with apply = 1: the images its removal takes
  std::vector<int32_t> carve_own;                 // and the owner frames' four counts
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

// The slot of `key`, or -1 when it is not in the table: dense_find's hash and probe without the CAS.  Nothing is claimed; at most n
// probes, ending at the first empty slot (slots keep their key until a purge, so a chain never loses a link).
__device__ __forceinline__ long long dense_lookup(const u64* keys, u64 n, u64 key) {
  u64 slot = dense_hash(key) & (n - 1);
  for (u64 it = 0; it < n; ++it) {
    const u64 cur = __hip_atomic_load(&keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == key) return (long long)slot;
    if (cur == kDenseEmpty) return -1;
    slot = (slot + 1) & (n - 1);
  }
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

struct DenseOutArgs {
  const u64* keys; DenseRec* rec; const u64* pkeys; const unsigned int* pcnt;
  u64 H, P;
  u64* ctr;
  u64* lkey; unsigned int* lval; u64 list_cap;          // compact
  const u64* skey; const unsigned int* sval; long long n_write;   // gather
  int with_color;
  int* okey; double* oxyz; int* ocnt; unsigned char* obgr; int* oinst; int* ovotes;   // null: not asked for
};

// The map's voxels as a list of (packed key, slot) in ascending key order, shared by esl_dense_extract and the six units that read
// the map.  A call's step: dense_list_begin, the caller's own buffers and the outputs it wants in L.k, dense_list_launch.
struct DenseList { DenseOutArgs k; size_t temp_bytes; };   // the kernels' arguments and the sort's temporary storage
// the list's buffers grown, the table pointers of L.k set (the rest zero), ctr[DC_LIST] cleared on the stream: outside every ProfScope
int dense_list_begin(esl_ctx* c, DenseState& d, DenseList& L);
// inside the caller's ProfScope: k_dense_compact, k_dense_vote when asked for, the radix sort and, when asked for, esl_dense_extract's
// gather of the first L.k.n_write (> 0) voxels of the sorted list into the non-null outputs of L.k (the readers point them at buffers
// of their own)
int dense_list_launch(esl_ctx* c, DenseState& d, DenseList& L, bool vote, bool gather);
// step 2 on the host: R and t of every frame, from the given poses or (cams == nullptr) the resident camera states; an invalid pose
// gives ESL_ERR_INVALID.  host / pose: the caller's staging vectors
int dense_frames_poses(esl_ctx* c, const char* who, const double* cams, int F, std::vector<double>& host, std::vector<double>& pose);

// esl_dense_planes' U_r: the indices i < n with state[i] == -2, ascending, into `list`, their number into *count (a stable rocprim
// select; with tmp == nullptr only tmp_bytes is set).  Defined in esl_dense.hip beside the list's sort, for the reason given there.
int dense_select_free(esl_ctx* c, void* tmp, size_t& tmp_bytes, const int* state, int* list, u64* count, size_t n);

inline int dense_fail(int rc, const char* who, const char* what) {
  set_error(std::string(who) + ": " + what);
  return rc;
}

// the state of a map that was begun, or null with the error set (the caller returns ESL_ERR_STATE)
inline DenseState* dense_begun(esl_ctx* c, const char* who) {
  if (c->dense && c->dense->begun) return c->dense;
  dense_fail(ESL_ERR_STATE, who, "no esl_dense_begin before");
  return nullptr;
}

inline unsigned dense_blocks(u64 n) { return (unsigned)((n + kDenseThreads - 1) / kDenseThreads); }

// a row of a unit's table of the buffers it grows, in order.  skip_empty: a row of 0 bytes is left alone (esl_dense_render and
// esl_dense_carve_frames: a buffer that this call has no use for); otherwise it is grown like any other, which gives an empty slot its
// 16 bytes and counts as an allocation (esl_dense_objects, esl_dense_planes, esl_dense_normals: every slot of theirs exists after a call)
struct DenseSlot { int slot; size_t bytes; };
template <int N, size_t R>
int dense_grow(esl_ctx* c, ScratchSet<N>& s, const DenseSlot (&want)[R], bool skip_empty) {
  for (const DenseSlot& w : want) {
    if (skip_empty && !w.bytes) continue;
    if (const int rc = s.grow(c, w.slot, w.bytes)) return rc;
  }
  return ESL_OK;
}

// an invalid map (over capacity or inconsistent): the result says so and the entry writes nothing more
template <class Result>
bool dense_map_invalid(const DenseState& d, Result* out) {
  if (!d.status) return false;
  out->status = d.status; out->n_voxels = -1;
  return true;
}

}  // namespace esl
