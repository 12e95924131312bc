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
//                     REMOVE (esl_dense_remove_frames / _move_frames, steps 8-11): the same kernel subtracting, by lookups that claim
//                     nothing.  A slot whose count reaches 0 is DEAD: it keeps its key (no probe chain loses a link) until a purge.
//   k_dense_audit     after every removing call, and after an add onto a map with dead slots: live and dead slots of both tables,
//                     and the inconsistencies that raise the sticky status 4
//   k_dense_export / _reinsert / _reinsert_pairs   esl_dense_purge: the tables rebuilt from the live records and pairs alone
//   k_dense_compact   extract: the live slots as (packed key, slot), appended with one atomic per wave; clears the best words
//   k_dense_vote      extract: per live pair one atomicMax of (votes << 32 | ~id) into its voxel's best word: most votes, ties to
//                     the lowest id.  Done at extract time over the whole pair table, so incremental adds stay exact.
//   rocprim radix sort of (packed key, slot), then k_dense_gather writes the first `cap` voxels in key order.
//   esl_dense_objects (include/esl.h, "per-instance ellipsoids from the dense map"; arithmetic: esl_dense_obj.hpp) works on that sorted
//   list: k_dobj_gate (kept voxels, totals, the forest), k_dobj_union (connected components: esl_uf.hpp's lock-free union-find over
//   neighbour probes of the voxel table), k_dobj_roots (real roots, size, samples), k_dobj_table (components of min_component voxels or
//   more); the host sorts the table and picks a component per label; k_dobj_rows / _box / _mom (integer moments of the chosen
//   components), the host builds their frames, k_dobj_ext (extents), k_dobj_vout (every voxel's table row).
//   esl_dense_planes (include/esl.h, "dominant planes and the ground from the dense map"; arithmetic: esl_dense_planes.hpp) works on
//   the same sorted list: k_dpl_gate (eligible voxels, their total and box); per round a stable rocprim select of the unassigned
//   eligible voxels (U_r), k_dpl_pack (centre and count of every entry, 32 bytes), k_dpl_gather (the keys of the hypotheses' entries;
//   the host builds the planes), k_dpl_score (every hypothesis against all of U_r: lane = hypothesis, the list staged in LDS tiles and
//   read by broadcast; with fewer than 64 hypotheses k_dpl_few scores them, lane = voxel) and k_dpl_one (one plane
//   against U_r, lane = voxel: the integer moments of its inliers, and their assignment);
//   k_dpl_vout (every voxel's plane).
// Every store to global memory is a vector store or an atomic in plain C++; no loop waits for another thread: a probe that finds no
// slot within the table's size, or a map over its capacity, raises the sticky status 3 and gives up.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "esl_ctx.hpp"
#include "esl_dense_key.hpp"
#include "esl_dense_obj.hpp"
#include "esl_dense_planes.hpp"
#include "esl_uf.hpp"

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

constexpr int kDenseThreads = 256;
constexpr int kDenseMaxVoxels = 1 << 26;
typedef unsigned long long u64;

struct DenseRec { long long S[3]; u64 col[3]; u64 count; u64 best; };
static_assert(sizeof(DenseRec) == 64, "one record per 64-byte segment");

// the device counters: this call's five counts, then what lives as long as the map
// (DC_VOXELS / DC_PAIRS count the slots CLAIMED since esl_dense_begin or the last purge), then a removing call's n_missing, the audit's
// five words and the purge's two list lengths
enum { DC_SAMPLED, DC_ZERO, DC_DEPTH_OUT, DC_KEY_OUT, DC_USED, DC_VOXELS, DC_PAIRS, DC_STATUS, DC_LIST,
       DC_MISSING, DC_LIVE_V, DC_DEAD_V, DC_LIVE_P, DC_DEAD_P, DC_BAD, DC_XV, DC_XP, DC_COUNT };

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
       DB_OKEY, DB_OXYZ, DB_OCNT, DB_OBGR, DB_OINST, DB_OVOTES,
       // esl_dense_objects
       DB_SIDX, DB_VLAB, DB_PARENT, DB_VROOT, DB_ROWOF, DB_CSIZE, DB_CSAMP, DB_OCTR, DB_LABKEPT, DB_TABLE, DB_ROWROOT, DB_ROWOBJ,
       DB_KBOX, DB_MOM, DB_AXES, DB_EXT, DB_VOUT,
       // esl_dense_planes
       DB_PSTATE, DB_PCTR, DB_PBOX, DB_PLIST, DB_PSELTMP, DB_PVOX, DB_PGKEY, DB_PPLANES, DB_PVALID, DB_PHACC, DB_PMOM, DB_PVOUT,
       // esl_dense_move_frames (the second pose set), esl_dense_purge (the live records and pairs)
       DB_POSE2, DB_XKEY, DB_XREC, DB_XPKEY, DB_XPID, DB_XPCNT, DB_COUNT };
struct DenseState {
  ScratchSet<DB_COUNT> set;
  bool begun = false, combine = true;
  esl_dense_params p;
  int with_color = 0, with_inst = 0;
  u64 H = 0;
  long long n_samples = 0, n_voxels = 0, n_pairs = 0;   // n_voxels, n_pairs: LIVE slots (what k_dense_compact lists, what votes)
  long long dead_voxels = 0, dead_pairs = 0;             // claimed slots whose count is 0 (steps 9 to 11); claimed = live + dead
  int status = 0;
  std::vector<double> cams, pose, cams2, pose2;   // host staging of a call's poses (esl_dense_move_frames: both sets)
  std::vector<int> moved;                         // esl_dense_move_frames: the frames whose pose changed
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

// grid = (blocks over the sampled pixels of a frame, frames: at most 65535, a workgroup takes blockIdx.y, + gridDim.y, ...)
// REMOVE (step 8): the same samples, formed the same way, subtract what they added.  The slots are looked up, never claimed
// (dense_lookup); every 64-bit sum takes the two's-complement negation of what the add takes, the pair count an atomicSub; a used
// sample that finds no voxel, or no pair, counts in ctr[DC_MISSING].  Every `REMOVE ? :` below is a compile-time choice: the add
// instantiations are the kernels they were, their atomics fire and forget.
template <bool COMBINE, bool REMOVE>
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
    bool miss = false;   // REMOVE: this lane's sample found no voxel, or no pair
    if (!COMBINE) {
      if (used) {
        slot = REMOVE ? dense_lookup(a.keys, a.H, key) : dense_find(a.keys, a.H, key, a.ctr, DC_VOXELS, a.max_voxels);
        if (REMOVE) miss = slot < 0;
        if (slot >= 0) {
          DenseRec* r = a.rec + slot;
          atomicAdd((u64*)&r->S[0], REMOVE ? 0ull - (u64)s0 : (u64)s0); atomicAdd((u64*)&r->S[1], REMOVE ? 0ull - (u64)s1 : (u64)s1);
          atomicAdd((u64*)&r->S[2], REMOVE ? 0ull - (u64)s2 : (u64)s2);
          atomicAdd(&r->count, REMOVE ? ~0ull : 1ull);
          if (a.bgr) {
            atomicAdd(&r->col[0], REMOVE ? 0ull - (rgbc & 0xFFFFull) : rgbc & 0xFFFFull);
            atomicAdd(&r->col[1], REMOVE ? 0ull - ((rgbc >> 16) & 0xFFFFull) : (rgbc >> 16) & 0xFFFFull);
            atomicAdd(&r->col[2], REMOVE ? 0ull - ((rgbc >> 32) & 0xFFFFull) : (rgbc >> 32) & 0xFFFFull);
          }
          if (a.pkeys && id >= 0) {
            const u64 pk = (u64)slot << 32 | (u64)(unsigned)id;
            const long long ps = REMOVE ? dense_lookup(a.pkeys, a.P, pk) : dense_find(a.pkeys, a.P, pk, a.ctr, DC_PAIRS, a.max_pairs);
            if (ps >= 0) { if (REMOVE) atomicSub(&a.pcnt[ps], 1u); else atomicAdd(&a.pcnt[ps], 1u); }
            else if (REMOVE) miss = true;
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
        slot = REMOVE ? dense_lookup(a.keys, a.H, key) : dense_find(a.keys, a.H, key, a.ctr, DC_VOXELS, a.max_voxels);
        if (slot >= 0) {
          DenseRec* r = a.rec + slot;
          atomicAdd((u64*)&r->S[0], REMOVE ? 0ull - (u64)s0 : (u64)s0); atomicAdd((u64*)&r->S[1], REMOVE ? 0ull - (u64)s1 : (u64)s1);
          atomicAdd((u64*)&r->S[2], REMOVE ? 0ull - (u64)s2 : (u64)s2);
          atomicAdd(&r->count, REMOVE ? 0ull - (rgbc >> 48) : rgbc >> 48);
          if (a.bgr) {
            atomicAdd(&r->col[0], REMOVE ? 0ull - (rgbc & 0xFFFFull) : rgbc & 0xFFFFull);
            atomicAdd(&r->col[1], REMOVE ? 0ull - ((rgbc >> 16) & 0xFFFFull) : (rgbc >> 16) & 0xFFFFull);
            atomicAdd(&r->col[2], REMOVE ? 0ull - ((rgbc >> 32) & 0xFFFFull) : (rgbc >> 32) & 0xFFFFull);
          }
        }
      }
      if (REMOVE || a.pkeys) {   // workgroup-uniform
        const int hl = 63 - __clzll((long long)(hm & le));   // the head of this lane's run; lane 0 is always a head
        const long long rslot = __shfl(slot, hl, 64);
        if (REMOVE) miss = used && rslot < 0;
        if (a.pkeys) {
          const bool vused = used && id >= 0 && rslot >= 0;
          const u64 vkey = vused ? ((u64)rslot << 32 | (u64)(unsigned)id) : kDenseEmpty;
          const u64 vprev = __shfl_up(vkey, 1, 64);
          const bool vhead = !vused || lane == 0 || vprev != vkey;
          const u64 vhm = __ballot(vhead);
          const int vrid = __popcll(vhm & le);
          const int votes = dense_run_sum(vused ? 1 : 0, vrid, lane);
          long long ps = 0;
          if (vused && vhead) {
            ps = REMOVE ? dense_lookup(a.pkeys, a.P, vkey) : dense_find(a.pkeys, a.P, vkey, a.ctr, DC_PAIRS, a.max_pairs);
            if (ps >= 0) { if (REMOVE) atomicSub(&a.pcnt[ps], (unsigned)votes); else atomicAdd(&a.pcnt[ps], (unsigned)votes); }
          }
          if (REMOVE) {   // every lane of a vote run whose head found no pair
            const long long hps = __shfl(ps, 63 - __clzll((long long)(vhm & le)), 64);
            miss = miss || (vused && hps < 0);
          }
        }
      }
    }
    if (REMOVE) {
      const u64 m_m = __ballot(miss);
      if (lane == 0 && m_m) atomicAdd(&a.ctr[DC_MISSING], (u64)__popcll(m_m));
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
  bool occ = key != kDenseEmpty;
  if (occ) a.rec[i].best = 0;
  occ = occ && a.rec[i].count != 0;   // a dead slot (step 9) keeps its key and is not listed
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
  const unsigned int votes = a.pcnt[i];
  if (votes == 0) return;   // a dead pair casts no vote (0 << 32 | ~id would still be a non-zero best word)
  if (slot < a.H) atomicMax(&a.rec[slot].best, (u64)votes << 32 | (u64)(unsigned)~(unsigned)key);
}

// Step 9's audit: one pass over the H voxel slots and the P pair slots, as at most kDenseAuditBlocks workgroups that stride over them.
// A lane keeps its five counts in registers, a wave folds them by a butterfly, the waves meet in LDS and one lane per count emits the
// workgroup's atomic.  live / dead: claimed slots with count > 0 / == 0.  bad: a voxel count negative as int64, a dead voxel with a
// non-zero S_a or colour sum, a pair count with bit 31 set, a live pair whose voxel is dead (or past the table).
constexpr int kDenseAuditBlocks = 1024;
static __global__ __launch_bounds__(kDenseThreads) void k_dense_audit(DenseOutArgs a) {
  __shared__ u64 part[kDenseThreads / 64][5];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const u64 n = a.pkeys ? (a.P > a.H ? a.P : a.H) : a.H, stride = (u64)gridDim.x * kDenseThreads;
  u64 v[5] = {0, 0, 0, 0, 0};   // live voxels, dead voxels, live pairs, dead pairs, bad
  for (u64 i = (u64)blockIdx.x * kDenseThreads + threadIdx.x; i < n; i += stride) {
    if (i < a.H && a.keys[i] != kDenseEmpty) {
      const DenseRec r = a.rec[i];
      const long long cnt = (long long)r.count;
      if (cnt > 0) ++v[0];
      else if (cnt < 0) ++v[4];
      else {
        ++v[1];
        if ((r.S[0] | r.S[1] | r.S[2]) != 0 || (r.col[0] | r.col[1] | r.col[2]) != 0) ++v[4];
      }
    }
    if (a.pkeys && i < a.P) {
      const u64 pk = a.pkeys[i];
      if (pk != kDenseEmpty) {
        const unsigned int pc = a.pcnt[i];
        if (pc >> 31) ++v[4];
        else if (pc == 0) ++v[3];
        else {
          ++v[2];
          const u64 slot = pk >> 32;
          if (slot >= a.H || a.rec[slot].count == 0) ++v[4];
        }
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int c = 0; c < 5; ++c) v[c] += __shfl_xor(v[c], off, 64);
  }
  if (lane == 0) {
    for (int c = 0; c < 5; ++c) part[wave][c] = v[c];
  }
  __syncthreads();
  if (threadIdx.x < 5) {
    u64 t = 0;
    for (int w = 0; w < kDenseThreads / 64; ++w) t += part[w][threadIdx.x];
    if (t) atomicAdd(&a.ctr[DC_LIVE_V + threadIdx.x], t);
  }
}

// esl_dense_purge (step 11).  k_dense_export appends the live records as (packed key, record) and the live pairs as (their voxel's
// packed key, id, count), one atomic per wave and list; the host clears the tables; k_dense_reinsert claims a slot per record (the
// keys are distinct: one CAS per probe, bounded by H) and stores it with vector stores; k_dense_reinsert_pairs, a launch later, looks
// the voxel's new slot up and claims the pair's.  No thread waits for another.
struct DensePurgeArgs {
  u64* keys; DenseRec* rec; u64* pkeys; unsigned int* pcnt;
  u64 H, P;
  u64* ctr;
  u64* xkey; DenseRec* xrec; u64 xv_cap;                          // the live records
  u64* xpkey; unsigned int* xpid; unsigned int* xpcnt; u64 xp_cap;   // the live pairs
};

static __global__ __launch_bounds__(kDenseThreads) void k_dense_export(DensePurgeArgs a) {
  const int lane = threadIdx.x & 63;
  const u64 below = (1ull << lane) - 1ull;
  const u64 i = (u64)blockIdx.x * kDenseThreads + threadIdx.x;
  {
    u64 key = kDenseEmpty;
    if (i < a.H) key = a.keys[i];
    const bool live = key != kDenseEmpty && a.rec[i].count != 0;
    const u64 m = __ballot(live);
    u64 base = 0;
    if (lane == 0 && m) base = atomicAdd(&a.ctr[DC_XV], (u64)__popcll(m));
    base = __shfl(base, 0, 64);
    if (live) {
      const u64 pos = base + (u64)__popcll(m & below);
      if (pos < a.xv_cap) { a.xkey[pos] = key; a.xrec[pos] = a.rec[i]; }
    }
  }
  if (a.pkeys) {   // workgroup-uniform
    u64 pk = kDenseEmpty;
    if (i < a.P) pk = a.pkeys[i];
    const bool live = pk != kDenseEmpty && a.pcnt[i] != 0 && (pk >> 32) < a.H;
    const u64 m = __ballot(live);
    u64 base = 0;
    if (lane == 0 && m) base = atomicAdd(&a.ctr[DC_XP], (u64)__popcll(m));
    base = __shfl(base, 0, 64);
    if (live) {
      const u64 pos = base + (u64)__popcll(m & below);
      if (pos < a.xp_cap) { a.xpkey[pos] = a.keys[pk >> 32]; a.xpid[pos] = (unsigned int)pk; a.xpcnt[pos] = a.pcnt[i]; }
    }
  }
}

// the slot claimed for `key`, which no other thread inserts, in an otherwise append-only table of n slots; -1 when none is free
__device__ __forceinline__ long long dense_claim(u64* keys, u64 n, u64 key) {
  u64 slot = dense_hash(key) & (n - 1);
  for (u64 it = 0; it < n; ++it) {
    if (atomicCAS(&keys[slot], kDenseEmpty, key) == kDenseEmpty) return (long long)slot;
    slot = (slot + 1) & (n - 1);
  }
  return -1;
}

static __global__ __launch_bounds__(kDenseThreads) void k_dense_reinsert(DensePurgeArgs a) {
  const u64 i = (u64)blockIdx.x * kDenseThreads + threadIdx.x;
  const u64 nv = a.ctr[DC_XV] < a.xv_cap ? a.ctr[DC_XV] : a.xv_cap;
  if (i >= nv) return;
  const long long slot = dense_claim(a.keys, a.H, a.xkey[i]);
  if (slot >= 0) a.rec[slot] = a.xrec[i];
}

static __global__ __launch_bounds__(kDenseThreads) void k_dense_reinsert_pairs(DensePurgeArgs a) {
  const u64 i = (u64)blockIdx.x * kDenseThreads + threadIdx.x;
  const u64 np = a.ctr[DC_XP] < a.xp_cap ? a.ctr[DC_XP] : a.xp_cap;
  if (i >= np) return;
  const long long slot = dense_lookup(a.keys, a.H, a.xpkey[i]);
  if (slot < 0) return;
  const long long ps = dense_claim(a.pkeys, a.P, (u64)slot << 32 | (u64)a.xpid[i]);
  if (ps >= 0) a.pcnt[ps] = a.xpcnt[i];
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

// ---- esl_dense_objects: the kernels (include/esl.h, "per-instance ellipsoids from the dense map") ------------------------------------------
// Voxel i is the i-th entry of the sorted list: ascending packed key, so the smallest index of a set is its smallest key.  The forest
// `parent` is over these indices and links the larger root under the smaller one: a component's final root IS its key's voxel.
enum { DO_IN_RANGE, DO_GATED, DO_KEPT, DO_COMP_ALL, DO_ROWS, DO_COUNT };
constexpr int kDobjRow = 8;   // a table row on the device: label, size, samples, root, kx, ky, kz, 0

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

// ---- esl_dense_planes: the kernels (include/esl.h, "dominant planes and the ground from the dense map") --------------------------------------
// state[i] of voxel i of the sorted list: -1 not eligible, -2 eligible and unassigned, p >= 0 assigned to plane p.  U_r is the list of
// the indices i with state -2, ascending (a stable select), and vox[j] the centre and count of its j-th entry.
enum { DP_ELIGIBLE, DP_NR, DP_COUNT };
constexpr int kDplTile = 512;       // entries of U_r per LDS tile of k_dpl_score: 16 KiB
constexpr int kDplGroup = 256;      // hypotheses per workgroup of k_dpl_score, one per lane
constexpr int kDplMaxChunks = 256;  // workgroups along the list
constexpr int kDplSmall = 64;       // fewer hypotheses than this (one wave) are scored by k_dpl_few, lane = voxel
struct DplVox { double x[3]; long long count; };
static_assert(sizeof(DplVox) == 32, "two 16-byte loads per entry");

struct DplFree {   // the select's predicate
  const int* state;
  __host__ __device__ bool operator()(int i) const { return state[i] == -2; }
};

struct DplArgs {
  const DenseRec* rec; u64 H;
  const u64* skey; const unsigned int* sval; int n;
  int* state;
  int min_count, skip_labelled;
  u64* ctr; int* box;                       // DP_*; kmin, kmax of the eligible voxels
  const int* list; DplVox* vox;             // U_r (its length: ctr[DP_NR]); n entries at most
  u64* gkeys; int n_hyp, round; u64 seed;   // 3 n_hyp packed keys
  const double* planes; const int* valid;   // n_hyp x 4; n_hyp
  u64* hacc;                                // n_hyp x 2: inlier voxels, inlier samples
  int n_r;
  double leaf, dist_tol;
  double one[4]; int assign; int kmin[3]; u64* mom;   // the one-plane pass: kDplMoments sums; assign >= 0: the inliers take this plane
  int* vout; long long n_vout;
};

// The two kernels with one target for all their sums (k_dpl_gate, k_dpl_one) run as at most kDplReduceBlocks workgroups that stride over
// the list: a lane keeps its sums in registers, a wave folds them by a butterfly, the workgroup's waves meet in LDS and one lane per
// sum emits the workgroup's atomic.  One atomic per WAVE and sum on the same few addresses cost 0.13 ms (k_dpl_one) and 0.48 ms
// (k_dpl_gate) per launch on the synthetic room's 435,533 voxels.
constexpr int kDplReduceBlocks = 512;
constexpr int kDplWaves = kDenseThreads / 64;

// step 1 over the sorted list
static __global__ __launch_bounds__(kDenseThreads) void k_dpl_gate(DplArgs a) {
  __shared__ int part[kDplWaves][7];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int cnt = 0;
  int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {INT_MIN, INT_MIN, INT_MIN};
  for (long long i = (long long)blockIdx.x * kDenseThreads + threadIdx.x; i < a.n; i += (long long)gridDim.x * kDenseThreads) {
    const unsigned int slot = a.sval[i];
    bool el = false;
    if (slot < a.H) {
      const u64 best = a.rec[slot].best, count = a.rec[slot].count;
      el = (long long)count >= (long long)a.min_count && !(a.skip_labelled && best != 0);
    }
    a.state[i] = el ? -2 : -1;
    if (el) {
      int k[3];
      dense_unpack(a.skey[i], k);
      for (int c = 0; c < 3; ++c) { lo[c] = min(lo[c], k[c]); hi[c] = max(hi[c], k[c]); }
      ++cnt;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    cnt += __shfl_xor(cnt, off, 64);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      lo[c] = min(lo[c], __shfl_xor(lo[c], off, 64));
      hi[c] = max(hi[c], __shfl_xor(hi[c], off, 64));
    }
  }
  if (lane == 0) {
    part[wave][0] = cnt;
    for (int c = 0; c < 3; ++c) { part[wave][1 + c] = lo[c]; part[wave][4 + c] = hi[c]; }
  }
  __syncthreads();
  if (threadIdx.x < 7) {
    const int c = threadIdx.x;
    int t = part[0][c];
    for (int w = 1; w < kDplWaves; ++w) t = c == 0 ? t + part[w][c] : c < 4 ? min(t, part[w][c]) : max(t, part[w][c]);
    if (c == 0) { if (t) atomicAdd(&a.ctr[DP_ELIGIBLE], (u64)t); }
    else if (c < 4) { if (t != INT_MAX) atomicMin(&a.box[c - 1], t); }
    else if (t != INT_MIN) atomicMax(&a.box[c - 1], t);
  }
}

// step 2: centre and count of every entry of U_r.  The grid covers n; the list's length is read on the device.
static __global__ __launch_bounds__(kDenseThreads) void k_dpl_pack(DplArgs a) {
  const long long j = (long long)blockIdx.x * kDenseThreads + threadIdx.x;
  const long long n_r = (long long)min(a.ctr[DP_NR], (u64)a.n);
  if (j >= n_r) return;
  const int i = a.list[j];
  if (i < 0 || i >= a.n) return;
  int k[3];
  dense_unpack(a.skey[i], k);
  const unsigned int slot = a.sval[i];
  DplVox v;
  for (int c = 0; c < 3; ++c) v.x[c] = dobj_center(k[c], a.leaf);
  v.count = slot < a.H ? (long long)a.rec[slot].count : 0;
  a.vox[j] = v;
}

// step 3: the packed keys of the entries i_0, i_1, i_2 of every hypothesis (all ones with fewer than three entries)
static __global__ __launch_bounds__(kDenseThreads) void k_dpl_gather(DplArgs a) {
  const int t = blockIdx.x * kDenseThreads + threadIdx.x;
  if (t >= 3 * a.n_hyp) return;
  const long long n_r = (long long)min(a.ctr[DP_NR], (u64)a.n);
  u64 key = kDenseEmpty;
  if (n_r >= 3) {
    const int i = a.list[dpl_index(a.seed, a.round, a.n_hyp, t / 3, t % 3, (int)n_r)];
    if (i >= 0 && i < a.n) key = a.skey[i];
  }
  a.gkeys[t] = key;
}

// step 4, the hot kernel.  Lane = hypothesis: its plane and its two sums stay in registers.  grid = (hypothesis groups, chunks of the
// list); a workgroup stages tile after tile of its chunk in LDS, and every lane reads every entry by broadcast.  Integer sums: the
// order of the chunks' atomics does not show.  An invalid hypothesis's lane runs along with a zero plane and adds nothing.  The host
// launches it for kDplSmall hypotheses or more only: below a wave most lanes would idle while every wave still walks every tile.
static __global__ __launch_bounds__(kDplGroup) void k_dpl_score(DplArgs a) {
  __shared__ DplVox tile[kDplTile];
  const int h = blockIdx.x * kDplGroup + threadIdx.x;
  const bool on = h < a.n_hyp && a.valid[h] != 0;
  double pl[4] = {0, 0, 0, 0};
  if (on) {
    for (int c = 0; c < 4; ++c) pl[c] = a.planes[(size_t)h * 4 + c];
  }
  unsigned int n_in = 0;
  u64 smp = 0;
  const int n_tiles = (a.n_r + kDplTile - 1) / kDplTile;
  for (int t = blockIdx.y; t < n_tiles; t += gridDim.y) {   // workgroup-uniform
    const int base = t * kDplTile, m = min(kDplTile, a.n_r - base);
    __syncthreads();   // the tile before this one has been read by every wave
    for (int j = threadIdx.x; j < m; j += kDplGroup) tile[j] = a.vox[base + j];
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < m; ++j) {
      const DplVox v = tile[j];
      const bool in = dpl_inlier(pl, v.x, a.dist_tol);
      n_in += in ? 1u : 0u;
      smp += in ? (u64)v.count : 0ull;
    }
  }
  if (on && n_in) {
    atomicAdd(&a.hacc[(size_t)h * 2], (u64)n_in);
    atomicAdd(&a.hacc[(size_t)h * 2 + 1], smp);
  }
}

// step 4 with fewer hypotheses than a wave (n_hyp < kDplSmall), where k_dpl_score's lanes would mostly idle: lane = voxel.  At most
// kDplReduceBlocks workgroups; hypothesis after hypothesis (workgroup-uniform) a lane strides over U_r with the two sums in registers,
// the wave folds them, the waves meet in LDS and one lane emits the workgroup's two atomics.  The list is read n_hyp times, from cache.
static __global__ __launch_bounds__(kDenseThreads) void k_dpl_few(DplArgs a) {
  __shared__ u64 part[kDplWaves][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int h = 0; h < a.n_hyp; ++h) {
    if (!a.valid[h]) continue;
    double pl[4];
    for (int c = 0; c < 4; ++c) pl[c] = a.planes[(size_t)h * 4 + c];
    u64 n_in = 0, smp = 0;
    for (long long j = (long long)blockIdx.x * kDenseThreads + threadIdx.x; j < a.n_r; j += (long long)gridDim.x * kDenseThreads) {
      const DplVox e = a.vox[j];
      const bool in = dpl_inlier(pl, e.x, a.dist_tol);
      n_in += in ? 1ull : 0ull;
      smp += in ? (u64)e.count : 0ull;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { n_in += __shfl_xor(n_in, off, 64); smp += __shfl_xor(smp, off, 64); }
    if (lane == 0) { part[wave][0] = n_in; part[wave][1] = smp; }
    __syncthreads();
    if (threadIdx.x < 2) {
      u64 t = 0;
      for (int w = 0; w < kDplWaves; ++w) t += part[w][threadIdx.x];
      if (t) atomicAdd(&a.hacc[(size_t)h * 2 + threadIdx.x], t);
    }
    __syncthreads();   // part is free again
  }
}

// steps 6 and 7: one plane against U_r, a lane per entry and stride.  The inliers' n, samples, s and M relative to kmin (64-bit integer
// sums); with assign >= 0 the inliers take that plane.
static __global__ __launch_bounds__(kDenseThreads) void k_dpl_one(DplArgs a) {
  __shared__ u64 part[kDplWaves][kDplMoments];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  u64 v[kDplMoments];
  for (int c = 0; c < kDplMoments; ++c) v[c] = 0;
  for (long long j = (long long)blockIdx.x * kDenseThreads + threadIdx.x; j < a.n_r; j += (long long)gridDim.x * kDenseThreads) {
    const DplVox e = a.vox[j];
    const int i = a.list[j];
    if (!dpl_inlier(a.one, e.x, a.dist_tol) || i < 0 || i >= a.n) continue;
    int k[3];
    dense_unpack(a.skey[i], k);
    const long long d0 = (long long)k[0] - a.kmin[0], d1 = (long long)k[1] - a.kmin[1], d2 = (long long)k[2] - a.kmin[2];
    v[0] += 1; v[1] += (u64)e.count; v[2] += (u64)d0; v[3] += (u64)d1; v[4] += (u64)d2;
    v[5] += (u64)(d0 * d0); v[6] += (u64)(d0 * d1); v[7] += (u64)(d0 * d2); v[8] += (u64)(d1 * d1); v[9] += (u64)(d1 * d2); v[10] += (u64)(d2 * d2);
    if (a.assign >= 0) a.state[i] = a.assign;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int c = 0; c < kDplMoments; ++c) v[c] += __shfl_xor(v[c], off, 64);
  }
  if (lane == 0) {
    for (int c = 0; c < kDplMoments; ++c) part[wave][c] = v[c];
  }
  __syncthreads();
  if (threadIdx.x < kDplMoments) {
    u64 t = 0;
    for (int w = 0; w < kDplWaves; ++w) t += part[w][threadIdx.x];
    if (t) atomicAdd(&a.mom[threadIdx.x], t);
  }
}

// step 8
static __global__ __launch_bounds__(kDenseThreads) void k_dpl_vout(DplArgs a) {
  const long long i = (long long)blockIdx.x * kDenseThreads + threadIdx.x;
  if (i >= a.n_vout) return;
  a.vout[i] = a.state[i];
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

// The map's voxels as a list of (packed key, slot) in ascending key order, shared by esl_dense_extract and esl_dense_objects.
// dense_list_grow: the list's buffers and the table pointers of `k`; dense_list_launch (inside the caller's ProfScope, after
// ctr[DC_LIST] was cleared on the stream): k_dense_compact, k_dense_vote when asked for, the radix sort.
int dense_list_grow(esl_ctx* c, DenseState& d, DenseOutArgs& k, size_t* temp_bytes) {
  ScratchSet<DB_COUNT>& s = d.set;
  const size_t n = (size_t)d.n_voxels;
  std::memset(&k, 0, sizeof(k));
  if (const int rc = s.grow(c, DB_LKEY, n * sizeof(u64))) return rc;
  if (const int rc = s.grow(c, DB_LVAL, n * sizeof(unsigned int))) return rc;
  if (const int rc = s.grow(c, DB_SKEY, n * sizeof(u64))) return rc;
  if (const int rc = s.grow(c, DB_SVAL, n * sizeof(unsigned int))) return rc;
  *temp_bytes = 0;
  ESL_HIP_TRY(rocprim::radix_sort_pairs(nullptr, *temp_bytes, s.at<u64>(DB_LKEY), s.at<u64>(DB_SKEY), s.at<unsigned int>(DB_LVAL),
                                        s.at<unsigned int>(DB_SVAL), n, 0, 63, c->stream));
  if (const int rc = s.grow(c, DB_TEMP, *temp_bytes)) return rc;
  k.keys = s.at<u64>(DB_KEYS); k.rec = s.at<DenseRec>(DB_REC);
  k.H = d.H; k.P = 2 * d.H; k.ctr = s.at<u64>(DB_CTR);
  k.lkey = s.at<u64>(DB_LKEY); k.lval = s.at<unsigned int>(DB_LVAL); k.list_cap = (u64)n;
  k.skey = s.at<u64>(DB_SKEY); k.sval = s.at<unsigned int>(DB_SVAL);
  return ESL_OK;
}

int dense_list_launch(esl_ctx* c, DenseState& d, DenseOutArgs& k, bool vote, size_t temp_bytes) {
  ScratchSet<DB_COUNT>& s = d.set;
  if (vote) { k.pkeys = s.at<u64>(DB_PKEYS); k.pcnt = s.at<unsigned int>(DB_PCNT); }
  hipLaunchKernelGGL(k_dense_compact, dim3(dense_blocks(k.H)), dim3(kDenseThreads), 0, c->stream, k);
  if (vote) hipLaunchKernelGGL(k_dense_vote, dim3(dense_blocks(k.P)), dim3(kDenseThreads), 0, c->stream, k);
  ESL_HIP_TRY(rocprim::radix_sort_pairs(s.buf[DB_TEMP], temp_bytes, s.at<u64>(DB_LKEY), s.at<u64>(DB_SKEY),
                                        s.at<unsigned int>(DB_LVAL), s.at<unsigned int>(DB_SVAL), (size_t)d.n_voxels, 0, 63, c->stream));
  return ESL_OK;
}

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
  d.n_samples = 0; d.n_voxels = 0; d.n_pairs = 0; d.dead_voxels = 0; d.dead_pairs = 0; d.status = 0;
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

namespace {

// what esl_dense_add_frames, _remove_frames and _move_frames check alike, case by case and in this order; res_cams: the poses (of
// _move_frames: the new ones) are the resident camera states
int dense_frames_check(esl_ctx* c, const char* who, int32_t F, const double K[4], int32_t rows, int32_t cols, const uint16_t* depth,
                       const uint8_t* bgr, const int32_t* inst, bool res_cams) {
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
  return resident_source_check(c, who, res_cams && F > 0, F, false, 0);
}

// step 2 on the host: R and t of every frame, from the given poses or the resident camera states
int dense_frames_poses(esl_ctx* c, const char* who, const double* cams, int F, std::vector<double>& host, std::vector<double>& pose) {
  host.resize((size_t)F * 7);
  if (cams) std::memcpy(host.data(), cams, (size_t)F * 7 * sizeof(double));
  else {
    ESL_HIP_TRY(hipMemcpyAsync(host.data(), c->cams, (size_t)F * 7 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    ESL_HIP_TRY(hipStreamSynchronize(c->stream));
  }
  pose.resize((size_t)F * kDensePose);
  for (int f = 0; f < F; ++f) {
    if (!dense_pose(host.data() + (size_t)f * 7, pose.data() + (size_t)f * kDensePose))
      return dense_fail(ESL_ERR_INVALID, who, "a pose with a non-finite number or a quaternion of norm 0");
  }
  return ESL_OK;
}

long long dense_per_frame(const DenseState& d, int rows, int cols) {
  return (long long)((rows + d.p.stride - 1) / d.p.stride) * ((cols + d.p.stride - 1) / d.p.stride);
}

// the kernel's arguments but the poses and the images
void dense_frames_args(DenseState& d, DenseArgs& k, int F, const double K[4], int rows, int cols) {
  ScratchSet<DB_COUNT>& s = d.set;
  std::memset(&k, 0, sizeof(k));
  k.F = F; k.rows = rows; k.cols = cols; k.stride = d.p.stride;
  k.srows = (rows + d.p.stride - 1) / d.p.stride; k.scols = (cols + d.p.stride - 1) / d.p.stride;
  for (int i = 0; i < 4; ++i) k.K[i] = K[i];
  k.leaf = d.p.leaf; k.depth_scale = d.p.depth_scale; k.depth_min = d.p.depth_min; k.depth_max = d.p.depth_max;
  k.keys = s.at<u64>(DB_KEYS); k.rec = s.at<DenseRec>(DB_REC);
  if (d.with_inst) { k.pkeys = s.at<u64>(DB_PKEYS); k.pcnt = s.at<unsigned int>(DB_PCNT); }
  k.H = d.H; k.P = 2 * d.H; k.max_voxels = (u64)d.p.max_voxels; k.max_pairs = 2 * (u64)d.p.max_voxels;
  k.ctr = s.at<u64>(DB_CTR);
}

// One pass of k_dense_insert over the frames of `k`, adding or removing, and what it means for the map.  k_dense_audit follows every
// removal, and an add while the map holds dead slots (a revived slot is no new claim: the claim counters no longer count the live
// ones); otherwise n_voxels and n_pairs come from the claim counters.  ctr: the device counters after the pass.
int dense_pass(esl_ctx* c, DenseState& d, const DenseArgs& k, bool remove, u64 ctr[DC_COUNT]) {
  const bool audit = remove || d.dead_voxels > 0 || d.dead_pairs > 0;
  ESL_HIP_TRY(hipMemsetAsync(k.ctr, 0, 5 * sizeof(u64), c->stream));   // this call's counts
  if (remove) ESL_HIP_TRY(hipMemsetAsync(k.ctr + DC_MISSING, 0, sizeof(u64), c->stream));
  if (audit) ESL_HIP_TRY(hipMemsetAsync(k.ctr + DC_LIVE_V, 0, 5 * sizeof(u64), c->stream));
  {
    ProfScope ps(c, 4);
    const dim3 grid(dense_blocks((u64)k.srows * (u64)k.scols), (unsigned)std::min(k.F, 65535));
    if (remove) {
      if (d.combine) hipLaunchKernelGGL((k_dense_insert<true, true>), grid, dim3(kDenseThreads), 0, c->stream, k);
      else hipLaunchKernelGGL((k_dense_insert<false, true>), grid, dim3(kDenseThreads), 0, c->stream, k);
    } else {
      if (d.combine) hipLaunchKernelGGL((k_dense_insert<true, false>), grid, dim3(kDenseThreads), 0, c->stream, k);
      else hipLaunchKernelGGL((k_dense_insert<false, false>), grid, dim3(kDenseThreads), 0, c->stream, k);
    }
    if (audit) {
      DenseOutArgs o;
      std::memset(&o, 0, sizeof(o));
      o.keys = k.keys; o.rec = k.rec; o.pkeys = k.pkeys; o.pcnt = k.pcnt; o.H = k.H; o.P = k.P; o.ctr = k.ctr;
      const u64 n = k.pkeys ? k.P : k.H;
      hipLaunchKernelGGL(k_dense_audit, dim3(std::min<unsigned>(dense_blocks(n), kDenseAuditBlocks)), dim3(kDenseThreads), 0, c->stream, o);
    }
  }
  ESL_HIP_TRY(hipGetLastError());
  ESL_HIP_TRY(hipMemcpyAsync(ctr, k.ctr, DC_COUNT * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  ESL_HIP_TRY(hipStreamSynchronize(c->stream));   // the caller's arrays are free again
  if (remove) d.n_samples -= (long long)ctr[DC_USED]; else d.n_samples += (long long)ctr[DC_USED];
  if (audit) {
    d.n_voxels = (long long)ctr[DC_LIVE_V]; d.n_pairs = (long long)ctr[DC_LIVE_P];
    d.dead_voxels = (long long)ctr[DC_DEAD_V]; d.dead_pairs = (long long)ctr[DC_DEAD_P];
  } else {
    d.n_voxels = (long long)ctr[DC_VOXELS]; d.n_pairs = (long long)ctr[DC_PAIRS];
  }
  d.status = ctr[DC_STATUS] ? 3 : (audit && (ctr[DC_BAD] || (remove && ctr[DC_MISSING]))) ? 4 : 0;
  return ESL_OK;
}

void dense_add_counts(const u64 ctr[DC_COUNT], int status, esl_dense_add_result* out) {
  out->n_sampled = (int64_t)ctr[DC_SAMPLED]; out->n_zero = (int64_t)ctr[DC_ZERO]; out->n_depth_out = (int64_t)ctr[DC_DEPTH_OUT];
  out->n_key_out = (int64_t)ctr[DC_KEY_OUT]; out->n_used = (int64_t)ctr[DC_USED]; out->status = status; out->pad = 0;
}

void dense_remove_counts(const u64 ctr[DC_COUNT], long long emptied, int status, esl_dense_remove_result* out) {
  out->n_sampled = (int64_t)ctr[DC_SAMPLED]; out->n_zero = (int64_t)ctr[DC_ZERO]; out->n_depth_out = (int64_t)ctr[DC_DEPTH_OUT];
  out->n_key_out = (int64_t)ctr[DC_KEY_OUT]; out->n_used = (int64_t)ctr[DC_USED]; out->n_missing = (int64_t)ctr[DC_MISSING];
  out->n_emptied = emptied; out->status = status; out->pad = 0;
}

void dense_slots_of(const DenseState& d, esl_dense_slots* out) {
  if (d.status) { out->voxel_slots = out->dead_voxels = out->pair_slots = out->dead_pairs = -1; return; }
  out->voxel_slots = d.n_voxels + d.dead_voxels; out->dead_voxels = d.dead_voxels;
  out->pair_slots = d.n_pairs + d.dead_pairs; out->dead_pairs = d.dead_pairs;
}

}  // namespace

extern "C" int esl_dense_add_frames(esl_ctx* c, const double* cams, int32_t F, const double K[4], int32_t rows, int32_t cols,
                                    const uint16_t* depth, const uint8_t* bgr, const int32_t* inst, esl_dense_add_result* out) {
  const char* who = "esl_dense_add_frames";
  if (const int rc = dense_frames_check(c, who, F, K, rows, cols, depth, bgr, inst, !cams)) return rc;
  DenseState& d = *c->dense;
  if (out) { std::memset(out, 0, sizeof(*out)); out->status = d.status; }
  if (F == 0 || d.status) return ESL_OK;   // nothing to add; or an invalid map: nothing more is added until the next esl_dense_begin
  ESL_HIP_TRY(hipSetDevice(c->device));
  // the poses: R and t of every frame on the host, before anything is added
  if (const int rc = dense_frames_poses(c, who, cams, F, d.cams, d.pose)) return rc;
  if (d.n_samples + dense_per_frame(d, rows, cols) * F >= (1ll << 31)) return dense_fail(ESL_ERR_INVALID, who, "n_samples would reach 2^31");
  ScratchSet<DB_COUNT>& s = d.set;
  const size_t n_img = (size_t)F * rows * cols;
  DenseArgs k;
  dense_frames_args(d, k, F, K, rows, cols);
  if (const int rc = upload(c, s, DB_POSE, (const double*)d.pose.data(), (size_t)F * kDensePose * sizeof(double), &k.pose)) return rc;
  if (const int rc = upload(c, s, DB_DEPTH, depth, n_img * sizeof(uint16_t), &k.depth)) return rc;
  if (d.with_color) { if (const int rc = upload(c, s, DB_BGR, bgr, n_img * 3, &k.bgr)) return rc; }
  if (d.with_inst) { if (const int rc = upload(c, s, DB_INST, inst, n_img * sizeof(int32_t), &k.inst)) return rc; }
  u64 ctr[DC_COUNT];
  if (const int rc = dense_pass(c, d, k, false, ctr)) return rc;
  if (out) dense_add_counts(ctr, d.status, out);
  return ESL_OK;
}

extern "C" int esl_dense_remove_frames(esl_ctx* c, const double* cams, int32_t F, const double K[4], int32_t rows, int32_t cols,
                                       const uint16_t* depth, const uint8_t* bgr, const int32_t* inst, esl_dense_remove_result* out) {
  const char* who = "esl_dense_remove_frames";
  if (const int rc = dense_frames_check(c, who, F, K, rows, cols, depth, bgr, inst, !cams)) return rc;
  DenseState& d = *c->dense;
  if (out) { std::memset(out, 0, sizeof(*out)); out->status = d.status; }
  if (F == 0 || d.status) return ESL_OK;   // nothing to remove; or an invalid map: nothing more is removed until the next esl_dense_begin
  ESL_HIP_TRY(hipSetDevice(c->device));
  if (const int rc = dense_frames_poses(c, who, cams, F, d.cams, d.pose)) return rc;
  if (dense_per_frame(d, rows, cols) * F >= (1ll << 31)) return dense_fail(ESL_ERR_INVALID, who, "more samples than a map holds: 2^31");
  ScratchSet<DB_COUNT>& s = d.set;
  const size_t n_img = (size_t)F * rows * cols;
  DenseArgs k;
  dense_frames_args(d, k, F, K, rows, cols);
  if (const int rc = upload(c, s, DB_POSE, (const double*)d.pose.data(), (size_t)F * kDensePose * sizeof(double), &k.pose)) return rc;
  if (const int rc = upload(c, s, DB_DEPTH, depth, n_img * sizeof(uint16_t), &k.depth)) return rc;
  if (d.with_color) { if (const int rc = upload(c, s, DB_BGR, bgr, n_img * 3, &k.bgr)) return rc; }
  if (d.with_inst) { if (const int rc = upload(c, s, DB_INST, inst, n_img * sizeof(int32_t), &k.inst)) return rc; }
  const long long dead_before = d.dead_voxels;
  u64 ctr[DC_COUNT];
  if (const int rc = dense_pass(c, d, k, true, ctr)) return rc;
  if (out) dense_remove_counts(ctr, d.dead_voxels - dead_before, d.status, out);
  return ESL_OK;
}

extern "C" int esl_dense_move_frames(esl_ctx* c, const double* cams_old, const double* cams_new, int32_t F, const double K[4], int32_t rows,
                                     int32_t cols, const uint16_t* depth, const uint8_t* bgr, const int32_t* inst,
                                     esl_dense_move_result* out) {
  const char* who = "esl_dense_move_frames";
  if (c && F > 0 && !cams_old) return dense_fail(ESL_ERR_INVALID, who, "null cams_old");
  if (const int rc = dense_frames_check(c, who, F, K, rows, cols, depth, bgr, inst, !cams_new)) return rc;
  DenseState& d = *c->dense;
  if (out) { std::memset(out, 0, sizeof(*out)); out->removed.status = out->added.status = d.status; }
  if (F == 0 || d.status) return ESL_OK;
  ESL_HIP_TRY(hipSetDevice(c->device));
  // every check before anything changes: all poses of both sets, then the frames that move and the samples they could add
  if (const int rc = dense_frames_poses(c, who, cams_new, F, d.cams2, d.pose2)) return rc;
  if (const int rc = dense_frames_poses(c, who, cams_old, F, d.cams, d.pose)) return rc;
  d.moved.clear();
  for (int f = 0; f < F; ++f) {
    if (std::memcmp(d.cams.data() + (size_t)f * 7, d.cams2.data() + (size_t)f * 7, 7 * sizeof(double)) != 0) d.moved.push_back(f);
  }
  const int Fm = (int)d.moved.size();
  if (d.n_samples + dense_per_frame(d, rows, cols) * Fm >= (1ll << 31)) return dense_fail(ESL_ERR_INVALID, who, "n_samples would reach 2^31");
  if (out) { out->n_frames_moved = Fm; out->n_frames_same = F - Fm; }
  if (Fm == 0) return ESL_OK;
  // the moved frames' poses and images, packed in their order and uploaded once
  for (int m = 0; m < Fm; ++m) {
    const size_t f = (size_t)d.moved[(size_t)m];
    if (f == (size_t)m) continue;
    std::memmove(d.pose.data() + (size_t)m * kDensePose, d.pose.data() + f * kDensePose, kDensePose * sizeof(double));
    std::memmove(d.pose2.data() + (size_t)m * kDensePose, d.pose2.data() + f * kDensePose, kDensePose * sizeof(double));
  }
  ScratchSet<DB_COUNT>& s = d.set;
  const size_t px = (size_t)rows * cols, n_img = (size_t)Fm * px;
  DenseArgs k;
  dense_frames_args(d, k, Fm, K, rows, cols);
  const double* pose_new = nullptr;
  if (const int rc = upload(c, s, DB_POSE, (const double*)d.pose.data(), (size_t)Fm * kDensePose * sizeof(double), &k.pose)) return rc;
  if (const int rc = upload(c, s, DB_POSE2, (const double*)d.pose2.data(), (size_t)Fm * kDensePose * sizeof(double), &pose_new)) return rc;
  if (const int rc = s.grow(c, DB_DEPTH, n_img * sizeof(uint16_t))) return rc;
  if (d.with_color) { if (const int rc = s.grow(c, DB_BGR, n_img * 3)) return rc; }
  if (d.with_inst) { if (const int rc = s.grow(c, DB_INST, n_img * sizeof(int32_t))) return rc; }
  for (int m = 0; m < Fm;) {   // one copy per run of consecutive frames
    int e = m + 1;
    while (e < Fm && d.moved[(size_t)e] == d.moved[(size_t)e - 1] + 1) ++e;
    const size_t f = (size_t)d.moved[(size_t)m], cnt = (size_t)(e - m) * px;
    ESL_HIP_TRY(hipMemcpyAsync(s.at<uint16_t>(DB_DEPTH) + (size_t)m * px, depth + f * px, cnt * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
    if (d.with_color) ESL_HIP_TRY(hipMemcpyAsync(s.at<uint8_t>(DB_BGR) + (size_t)m * px * 3, bgr + f * px * 3, cnt * 3, hipMemcpyHostToDevice, c->stream));
    if (d.with_inst) ESL_HIP_TRY(hipMemcpyAsync(s.at<int32_t>(DB_INST) + (size_t)m * px, inst + f * px, cnt * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    m = e;
  }
  k.depth = s.at<unsigned short>(DB_DEPTH);
  if (d.with_color) k.bgr = s.at<unsigned char>(DB_BGR);
  if (d.with_inst) k.inst = s.at<int>(DB_INST);
  const long long dead_before = d.dead_voxels;
  u64 ctr[DC_COUNT];
  if (const int rc = dense_pass(c, d, k, true, ctr)) return rc;
  if (out) dense_remove_counts(ctr, d.dead_voxels - dead_before, d.status, &out->removed);
  if (d.status) {   // the removal left an inconsistent map: nothing is added
    if (out) out->added.status = d.status;
    return ESL_OK;
  }
  k.pose = pose_new;
  if (const int rc = dense_pass(c, d, k, false, ctr)) return rc;
  if (out) dense_add_counts(ctr, d.status, &out->added);
  return ESL_OK;
}

extern "C" int esl_dense_slots_get(esl_ctx* c, esl_dense_slots* out) {
  const char* who = "esl_dense_slots_get";
  if (!c || !out) return dense_fail(ESL_ERR_INVALID, who, "null pointer");
  if (!c->dense || !c->dense->begun) return dense_fail(ESL_ERR_STATE, who, "no esl_dense_begin before");
  dense_slots_of(*c->dense, out);
  return ESL_OK;
}

extern "C" int esl_dense_purge(esl_ctx* c, esl_dense_slots* before, esl_dense_slots* after) {
  const char* who = "esl_dense_purge";
  if (!c) return dense_fail(ESL_ERR_INVALID, who, "null ctx");
  if (!c->dense || !c->dense->begun) return dense_fail(ESL_ERR_STATE, who, "no esl_dense_begin before");
  DenseState& d = *c->dense;
  if (before) dense_slots_of(d, before);
  if (after) dense_slots_of(d, after);
  if (d.status || (d.dead_voxels == 0 && d.dead_pairs == 0)) return ESL_OK;   // an invalid map is left alone; nothing dead: nothing to do
  ESL_HIP_TRY(hipSetDevice(c->device));
  ScratchSet<DB_COUNT>& s = d.set;
  const size_t nv = (size_t)d.n_voxels, np = d.with_inst ? (size_t)d.n_pairs : 0, H = (size_t)d.H;
  if (const int rc = s.grow(c, DB_XKEY, nv * sizeof(u64))) return rc;
  if (const int rc = s.grow(c, DB_XREC, nv * sizeof(DenseRec))) return rc;
  if (const int rc = s.grow(c, DB_XPKEY, np * sizeof(u64))) return rc;
  if (const int rc = s.grow(c, DB_XPID, np * sizeof(unsigned int))) return rc;
  if (const int rc = s.grow(c, DB_XPCNT, np * sizeof(unsigned int))) return rc;
  DensePurgeArgs a;
  std::memset(&a, 0, sizeof(a));
  a.keys = s.at<u64>(DB_KEYS); a.rec = s.at<DenseRec>(DB_REC);
  if (d.with_inst) { a.pkeys = s.at<u64>(DB_PKEYS); a.pcnt = s.at<unsigned int>(DB_PCNT); }
  a.H = d.H; a.P = 2 * d.H; a.ctr = s.at<u64>(DB_CTR);
  a.xkey = s.at<u64>(DB_XKEY); a.xrec = s.at<DenseRec>(DB_XREC); a.xv_cap = (u64)nv;
  a.xpkey = s.at<u64>(DB_XPKEY); a.xpid = s.at<unsigned int>(DB_XPID); a.xpcnt = s.at<unsigned int>(DB_XPCNT); a.xp_cap = (u64)np;
  const u64 claimed[2] = {(u64)nv, (u64)np};   // DC_VOXELS, DC_PAIRS: afterwards claimed = live
  ESL_HIP_TRY(hipMemsetAsync(a.ctr + DC_XV, 0, 2 * sizeof(u64), c->stream));
  {
    ProfScope ps(c, 4);
    hipLaunchKernelGGL(k_dense_export, dim3(dense_blocks(d.with_inst ? a.P : a.H)), dim3(kDenseThreads), 0, c->stream, a);
    ESL_HIP_TRY(hipMemsetAsync(s.buf[DB_KEYS], 0xFF, H * sizeof(u64), c->stream));
    ESL_HIP_TRY(hipMemsetAsync(s.buf[DB_REC], 0, H * sizeof(DenseRec), c->stream));
    if (d.with_inst) {
      ESL_HIP_TRY(hipMemsetAsync(s.buf[DB_PKEYS], 0xFF, 2 * H * sizeof(u64), c->stream));
      ESL_HIP_TRY(hipMemsetAsync(s.buf[DB_PCNT], 0, 2 * H * sizeof(unsigned int), c->stream));
    }
    if (nv) hipLaunchKernelGGL(k_dense_reinsert, dim3(dense_blocks((u64)nv)), dim3(kDenseThreads), 0, c->stream, a);
    if (np) hipLaunchKernelGGL(k_dense_reinsert_pairs, dim3(dense_blocks((u64)np)), dim3(kDenseThreads), 0, c->stream, a);
  }
  ESL_HIP_TRY(hipGetLastError());
  ESL_HIP_TRY(hipMemcpyAsync(a.ctr + DC_VOXELS, claimed, sizeof(claimed), hipMemcpyHostToDevice, c->stream));
  ESL_HIP_TRY(hipStreamSynchronize(c->stream));
  d.dead_voxels = 0; d.dead_pairs = 0;
  if (after) dense_slots_of(d, after);
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
  if (d.status) { *n_voxels = -1; return ESL_OK; }   // over capacity or inconsistent: the map is invalid, nothing is written
  *n_voxels = d.n_voxels;
  const long long n = d.n_voxels, nw = std::min<long long>(n, cap);
  const bool any = key_out || xyz_out || count_out || bgr_out || inst_out || votes_out;
  if (nw == 0 || !any) return ESL_OK;
  ESL_HIP_TRY(hipSetDevice(c->device));
  ScratchSet<DB_COUNT>& s = d.set;
  DenseOutArgs k;
  size_t temp_bytes = 0;
  if (const int rc = dense_list_grow(c, d, k, &temp_bytes)) return rc;
  if (key_out) { if (const int rc = s.grow(c, DB_OKEY, (size_t)nw * 3 * sizeof(int32_t))) return rc; k.okey = s.at<int>(DB_OKEY); }
  if (xyz_out) { if (const int rc = s.grow(c, DB_OXYZ, (size_t)nw * 3 * sizeof(double))) return rc; k.oxyz = s.at<double>(DB_OXYZ); }
  if (count_out) { if (const int rc = s.grow(c, DB_OCNT, (size_t)nw * sizeof(int32_t))) return rc; k.ocnt = s.at<int>(DB_OCNT); }
  if (bgr_out) { if (const int rc = s.grow(c, DB_OBGR, (size_t)nw * 3)) return rc; k.obgr = s.at<unsigned char>(DB_OBGR); }
  if (inst_out) { if (const int rc = s.grow(c, DB_OINST, (size_t)nw * sizeof(int32_t))) return rc; k.oinst = s.at<int>(DB_OINST); }
  if (votes_out) { if (const int rc = s.grow(c, DB_OVOTES, (size_t)nw * sizeof(int32_t))) return rc; k.ovotes = s.at<int>(DB_OVOTES); }
  k.n_write = nw;
  k.with_color = d.with_color;
  const bool vote = d.with_inst && (inst_out || votes_out);
  ESL_HIP_TRY(hipMemsetAsync(k.ctr + DC_LIST, 0, sizeof(u64), c->stream));
  {
    ProfScope ps(c, 4);
    if (const int rc = dense_list_launch(c, d, k, vote, temp_bytes)) return rc;
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

// ---- esl_dense_objects ----------------------------------------------------------------------------------------------------------------------
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
  if (!c->dense || !c->dense->begun) return dense_fail(ESL_ERR_STATE, who, "no esl_dense_begin before");
  DenseState& d = *c->dense;
  if (!d.with_inst) return dense_fail(ESL_ERR_STATE, who, "the map was begun without labels");
  std::memset(out, 0, sizeof(*out));
  if (d.status) { out->status = d.status; out->n_voxels = -1; return ESL_OK; }   // over capacity or inconsistent: the map is invalid, nothing is written
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
  ScratchSet<DB_COUNT>& s = d.set;
  DenseOutArgs k;
  size_t temp_bytes = 0;
  if (const int rc = dense_list_grow(c, d, k, &temp_bytes)) return rc;
  const long long table_cap = std::min<long long>(p.max_components, n);
  {
    const size_t sn = (size_t)n, sN = (size_t)N, st = (size_t)table_cap;
    const int slot[] = {DB_SIDX, DB_VLAB, DB_PARENT, DB_VROOT, DB_ROWOF, DB_CSIZE, DB_CSAMP, DB_OCTR, DB_LABKEPT, DB_TABLE, DB_ROWROOT,
                        DB_ROWOBJ, DB_KBOX, DB_MOM, DB_AXES, DB_EXT, DB_VOUT};
    const size_t bytes[] = {(size_t)d.H * 4, sn * 4, sn * 4, sn * 4, sn * 4, sn * 4, sn * 4, DO_COUNT * sizeof(u64), sN * 4,
                            st * kDobjRow * 4, st * 4, st * 4, sN * 6 * 4, sN * kDobjMoments * 8, sN * 9 * 8, sN * 6 * 8, (size_t)n_vox_w * 4};
    for (int i = 0; i < (int)(sizeof(slot) / sizeof(slot[0])); ++i)
      if (const int rc = s.grow(c, slot[i], bytes[i])) return rc;
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
  ESL_HIP_TRY(hipMemsetAsync(k.ctr + DC_LIST, 0, sizeof(u64), c->stream));
  ESL_HIP_TRY(hipMemsetAsync(a.ctr, 0, DO_COUNT * sizeof(u64), c->stream));
  if (N > 0) ESL_HIP_TRY(hipMemsetAsync(a.labkept, 0, (size_t)N * 4, c->stream));
  {
    ProfScope ps(c, 4);
    if (const int rc = dense_list_launch(c, d, k, true, temp_bytes)) return rc;
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
  std::vector<int> order((size_t)R);
  for (long long r = 0; r < R; ++r) order[(size_t)r] = (int)r;
  std::sort(order.begin(), order.end(), [&](int x, int y) {
    const int* tx = tab.data() + (size_t)x * kDobjRow; const int* ty = tab.data() + (size_t)y * kDobjRow;
    if (tx[0] != ty[0]) return tx[0] < ty[0];
    if (tx[1] != ty[1]) return tx[1] > ty[1];
    return tx[3] < ty[3];   // the root's index: the order of the packed keys
  });
  std::vector<int> rowroot((size_t)R), rowobj((size_t)R, -1), chosen((size_t)N, -1), nrows((size_t)N, 0);
  for (long long r = 0; r < R; ++r) {
    const int* t = tab.data() + (size_t)order[(size_t)r] * kDobjRow;
    rowroot[(size_t)r] = t[3];
    ++nrows[(size_t)t[0]];
    if (chosen[(size_t)t[0]] < 0) { chosen[(size_t)t[0]] = (int)r; rowobj[(size_t)r] = t[0]; }
    if (r < n_comp_w_max) {
      int32_t* co = comp_out + 6 * r;
      co[0] = t[0]; co[1] = t[1]; co[2] = t[2]; co[3] = t[4]; co[4] = t[5]; co[5] = t[6];
    }
  }
  std::vector<int> kbox((size_t)N * 6);
  for (int o = 0; o < N; ++o) for (int e = 0; e < 6; ++e) kbox[(size_t)o * 6 + e] = e < 3 ? INT_MAX : INT_MIN;
  if (R > 0) {
    ESL_HIP_TRY(hipMemcpyAsync(s.buf[DB_ROWROOT], rowroot.data(), (size_t)R * 4, hipMemcpyHostToDevice, c->stream));
    ESL_HIP_TRY(hipMemcpyAsync(s.buf[DB_ROWOBJ], rowobj.data(), (size_t)R * 4, hipMemcpyHostToDevice, c->stream));
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
    if (labkept[(size_t)o] == 0) { status[(size_t)o] = 1; continue; }
    if (chosen[(size_t)o] < 0) { status[(size_t)o] = 2; continue; }
    const int* kb = kbox.data() + (size_t)o * 6;
    long long span = 1;
    for (int e = 0; e < 3; ++e) span = std::max<long long>(span, (long long)kb[3 + e] - kb[e] + 1);
    const long long size = tab[(size_t)order[(size_t)chosen[(size_t)o]] * kDobjRow + 1];
    if (dobj_guard(size, span)) { status[(size_t)o] = 6; continue; }
    dobj_frame(pl, size, mom.data() + (size_t)o * kDobjMoments, axes.data() + (size_t)o * 9);
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
    const int st = status[(size_t)o], row = chosen[(size_t)o];
    if (st == 0) {
      double mn[3], mx[3];
      for (int e = 0; e < 3; ++e) { mn[e] = dobj_dec(ext[(size_t)o * 6 + e]); mx[e] = dobj_dec(ext[(size_t)o * 6 + 3 + e]); }
      dobj_row(axes.data() + (size_t)o * 9, mn, mx, d.p.leaf, objs_out + (size_t)o * 10);
      ++out->n_ok;
    }
    if (stats_out) {
      int32_t* so = stats_out + 6 * o;
      const int* t = row >= 0 ? tab.data() + (size_t)order[(size_t)row] * kDobjRow : nullptr;
      so[0] = st; so[1] = labkept[(size_t)o]; so[2] = nrows[(size_t)o]; so[3] = row; so[4] = t ? t[1] : 0; so[5] = t ? t[2] : 0;
    }
  }
  return ESL_OK;
}

// ---- esl_dense_planes -----------------------------------------------------------------------------------------------------------------------
extern "C" void esl_dense_plane_params_default(esl_dense_plane_params* p) {
  if (!p) return;
  p->dist_tol = 0.02; p->up[0] = p->up[1] = p->up[2] = 0; p->up_min_cos = 0.7071067811865476;
  p->n_hypotheses = 1024; p->max_planes = 8; p->min_inliers = 1000; p->min_baseline = 8; p->min_count = 1; p->skip_labelled = 0;
  p->refine = 1; p->pad = 0; p->seed = 0;
}

extern "C" int esl_debug_dense_planes_layout(int32_t* tile_out, int32_t* group_out) {
  if (!tile_out || !group_out) return dense_fail(ESL_ERR_INVALID, "esl_debug_dense_planes_layout", "null pointer");
  *tile_out = kDplTile; *group_out = kDplGroup;
  return ESL_OK;
}

namespace {

// one launch of k_dpl_one and its eleven sums on the host (a host round trip)
int dpl_one_pass(esl_ctx* c, DplArgs& a, const double pl[4], int assign, long long mom[kDplMoments]) {
  for (int e = 0; e < 4; ++e) a.one[e] = pl[e];
  a.assign = assign;
  ESL_HIP_TRY(hipMemsetAsync(a.mom, 0, kDplMoments * sizeof(u64), c->stream));
  {
    ProfScope ps(c, 4);
    hipLaunchKernelGGL(k_dpl_one, dim3(std::min<unsigned>(dense_blocks((u64)a.n_r), kDplReduceBlocks)), dim3(kDenseThreads), 0, c->stream, a);
  }
  ESL_HIP_TRY(hipGetLastError());
  ESL_HIP_TRY(hipMemcpyAsync(mom, a.mom, kDplMoments * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  ESL_HIP_TRY(hipStreamSynchronize(c->stream));
  return ESL_OK;
}

}  // namespace

extern "C" int esl_dense_planes(esl_ctx* c, const esl_dense_plane_params* pp, double* planes_out, double* centroid_out, int32_t* stats_out,
                                int64_t* samples_out, double* ground_out, int64_t voxel_cap, int32_t* voxel_plane_out, int64_t* hyp_out,
                                esl_dense_plane_result* out) {
  const char* who = "esl_dense_planes";
  if (!c) return dense_fail(ESL_ERR_INVALID, who, "null ctx");
  if (!out) return dense_fail(ESL_ERR_INVALID, who, "null out");
  if (!planes_out) return dense_fail(ESL_ERR_INVALID, who, "null planes_out");
  if (voxel_cap < 0) return dense_fail(ESL_ERR_INVALID, who, "negative voxel_cap");
  if (voxel_cap > 0 && !voxel_plane_out) return dense_fail(ESL_ERR_INVALID, who, "null voxel_plane_out with voxel_cap > 0");
  esl_dense_plane_params p;
  if (pp) p = *pp; else esl_dense_plane_params_default(&p);
  if (!std::isfinite(p.dist_tol) || !(p.dist_tol > 0)) return dense_fail(ESL_ERR_INVALID, who, "dist_tol not finite or <= 0");
  if (!dpl_up_valid(p.up)) return dense_fail(ESL_ERR_INVALID, who, "up not finite, or neither zero nor longer than 1e-12");
  if (!(p.up_min_cos >= 0 && p.up_min_cos <= 1)) return dense_fail(ESL_ERR_INVALID, who, "up_min_cos outside 0 .. 1");
  if (p.n_hypotheses < 1 || p.n_hypotheses > 65536) return dense_fail(ESL_ERR_INVALID, who, "n_hypotheses outside 1 .. 65536");
  if (p.max_planes < 1 || p.max_planes > 64) return dense_fail(ESL_ERR_INVALID, who, "max_planes outside 1 .. 64");
  if (p.min_inliers < 3) return dense_fail(ESL_ERR_INVALID, who, "min_inliers < 3");
  if (p.min_baseline < 1) return dense_fail(ESL_ERR_INVALID, who, "min_baseline < 1");
  if ((long long)p.max_planes * p.n_hypotheses >= (1ll << 31)) return dense_fail(ESL_ERR_INVALID, who, "max_planes n_hypotheses reaches 2^31");
  if (!c->dense || !c->dense->begun) return dense_fail(ESL_ERR_STATE, who, "no esl_dense_begin before");
  DenseState& d = *c->dense;
  std::memset(out, 0, sizeof(*out));
  if (d.status) { out->status = d.status; out->n_voxels = -1; return ESL_OK; }   // over capacity or inconsistent: the map is invalid, nothing is written
  const long long n = d.n_voxels, n_vox_w = std::min<long long>(n, voxel_cap);
  const int Hn = p.n_hypotheses, P = p.max_planes;
  out->n_voxels = (int32_t)n; out->ground_index = -1; out->stop_reason = 1;
  for (int i = 0; i < P * 4; ++i) planes_out[i] = 0;
  if (centroid_out) for (int i = 0; i < P * 3; ++i) centroid_out[i] = 0;
  if (stats_out) for (int i = 0; i < P * 8; ++i) stats_out[i] = 0;
  if (samples_out) for (int i = 0; i < P; ++i) samples_out[i] = 0;
  if (ground_out) for (int i = 0; i < 4; ++i) ground_out[i] = 0;
  if (hyp_out) std::memset(hyp_out, 0, (size_t)P * Hn * 3 * sizeof(int64_t));
  if (n == 0) return ESL_OK;   // step 2 with n_0 = 0

  ESL_HIP_TRY(hipSetDevice(c->device));
  ScratchSet<DB_COUNT>& s = d.set;
  DenseOutArgs k;
  size_t temp_bytes = 0, sel_bytes = 0;
  if (const int rc = dense_list_grow(c, d, k, &temp_bytes)) return rc;
  {
    const size_t sn = (size_t)n, sh = (size_t)Hn;
    const int slot[] = {DB_PSTATE, DB_PCTR, DB_PBOX, DB_PLIST, DB_PVOX, DB_PGKEY, DB_PPLANES, DB_PVALID, DB_PHACC, DB_PMOM, DB_PVOUT};
    const size_t bytes[] = {sn * 4, DP_COUNT * sizeof(u64), 6 * 4, sn * 4, sn * sizeof(DplVox), sh * 3 * 8, sh * 4 * 8, sh * 4, sh * 2 * 8,
                            kDplMoments * sizeof(u64), (size_t)n_vox_w * 4};
    for (int i = 0; i < (int)(sizeof(slot) / sizeof(slot[0])); ++i)
      if (const int rc = s.grow(c, slot[i], bytes[i])) return rc;
  }
  DplArgs a;
  std::memset(&a, 0, sizeof(a));
  a.rec = k.rec; a.H = k.H; a.skey = k.skey; a.sval = k.sval; a.n = (int)n;
  a.state = s.at<int>(DB_PSTATE); a.min_count = p.min_count; a.skip_labelled = p.skip_labelled != 0;
  a.ctr = s.at<u64>(DB_PCTR); a.box = s.at<int>(DB_PBOX);
  a.list = s.at<int>(DB_PLIST); a.vox = s.at<DplVox>(DB_PVOX);
  a.gkeys = s.at<u64>(DB_PGKEY); a.n_hyp = Hn; a.seed = p.seed;
  a.planes = s.at<double>(DB_PPLANES); a.valid = s.at<int>(DB_PVALID); a.hacc = s.at<u64>(DB_PHACC);
  a.leaf = d.p.leaf; a.dist_tol = p.dist_tol; a.mom = s.at<u64>(DB_PMOM);
  a.vout = s.at<int>(DB_PVOUT); a.n_vout = n_vox_w;
  const DplFree is_free{a.state};
  ESL_HIP_TRY(rocprim::select(nullptr, sel_bytes, rocprim::counting_iterator<int>(0), s.at<int>(DB_PLIST), a.ctr + DP_NR, (size_t)n, is_free,
                              c->stream));
  if (const int rc = s.grow(c, DB_PSELTMP, sel_bytes)) return rc;
  const dim3 blk(kDenseThreads), grid_n(dense_blocks((u64)n));

  // step 1
  int box[6] = {INT_MAX, INT_MAX, INT_MAX, INT_MIN, INT_MIN, INT_MIN};
  u64 ctr[DP_COUNT];
  ESL_HIP_TRY(hipMemsetAsync(k.ctr + DC_LIST, 0, sizeof(u64), c->stream));
  ESL_HIP_TRY(hipMemsetAsync(a.ctr, 0, DP_COUNT * sizeof(u64), c->stream));
  ESL_HIP_TRY(hipMemcpyAsync(a.box, box, sizeof(box), hipMemcpyHostToDevice, c->stream));
  {
    ProfScope ps(c, 4);
    if (const int rc = dense_list_launch(c, d, k, d.with_inst && a.skip_labelled, temp_bytes)) return rc;
    hipLaunchKernelGGL(k_dpl_gate, dim3(std::min<unsigned>(dense_blocks((u64)n), kDplReduceBlocks)), blk, 0, c->stream, a);
  }
  ESL_HIP_TRY(hipGetLastError());
  ESL_HIP_TRY(hipMemcpyAsync(ctr, a.ctr, sizeof(ctr), hipMemcpyDeviceToHost, c->stream));
  ESL_HIP_TRY(hipMemcpyAsync(box, a.box, sizeof(box), hipMemcpyDeviceToHost, c->stream));
  ESL_HIP_TRY(hipStreamSynchronize(c->stream));
  out->n_eligible = (int32_t)ctr[DP_ELIGIBLE];
  long long span = 1;
  if (ctr[DP_ELIGIBLE] > 0) {
    for (int e = 0; e < 3; ++e) { span = std::max<long long>(span, (long long)box[3 + e] - box[e] + 1); a.kmin[e] = box[e]; }
  }

  std::vector<u64> gkeys((size_t)Hn * 3), hacc((size_t)Hn * 2);
  std::vector<double> planes((size_t)Hn * 4);
  std::vector<int> valid((size_t)Hn);
  std::vector<int32_t> plane_in;   // the reported planes' inlier voxels (the ground choice)
  const unsigned groups = (unsigned)((Hn + kDplGroup - 1) / kDplGroup);
  int stop = 0;
  for (int r = 0; r < P; ++r) {
    // step 2: U_r, its entries' centres and counts, and the keys of the hypotheses' entries
    a.round = r;
    {
      ProfScope ps(c, 4);
      ESL_HIP_TRY(rocprim::select(s.buf[DB_PSELTMP], sel_bytes, rocprim::counting_iterator<int>(0), s.at<int>(DB_PLIST), a.ctr + DP_NR, (size_t)n,
                                  is_free, c->stream));
      hipLaunchKernelGGL(k_dpl_pack, grid_n, blk, 0, c->stream, a);
      hipLaunchKernelGGL(k_dpl_gather, dim3(dense_blocks((u64)Hn * 3)), blk, 0, c->stream, a);
    }
    ESL_HIP_TRY(hipGetLastError());
    ESL_HIP_TRY(hipMemcpyAsync(ctr, a.ctr, sizeof(ctr), hipMemcpyDeviceToHost, c->stream));
    ESL_HIP_TRY(hipMemcpyAsync(gkeys.data(), a.gkeys, gkeys.size() * 8, hipMemcpyDeviceToHost, c->stream));
    ESL_HIP_TRY(hipStreamSynchronize(c->stream));
    const long long n_r = (long long)std::min<u64>(ctr[DP_NR], (u64)n);
    if (n_r < 3) { stop = 1; break; }
    a.n_r = (int)n_r;
    out->rounds = r + 1;
    // step 3 on the host
    int n_valid = 0;
    for (int h = 0; h < Hn; ++h) {
      int idx[3], key[3][3];
      for (int e = 0; e < 3; ++e) { idx[e] = dpl_index(p.seed, r, Hn, h, e, (int)n_r); dense_unpack(gkeys[(size_t)h * 3 + e], key[e]); }
      valid[(size_t)h] = dpl_hypothesis(idx, key[0], key[1], key[2], p.min_baseline, d.p.leaf, planes.data() + (size_t)h * 4) ? 1 : 0;
      n_valid += valid[(size_t)h];
    }
    if (n_valid == 0) { stop = 2; break; }   // the round's rows of hyp_out stay zero
    // step 4
    ESL_HIP_TRY(hipMemcpyAsync(s.buf[DB_PPLANES], planes.data(), planes.size() * 8, hipMemcpyHostToDevice, c->stream));
    ESL_HIP_TRY(hipMemcpyAsync(s.buf[DB_PVALID], valid.data(), valid.size() * 4, hipMemcpyHostToDevice, c->stream));
    ESL_HIP_TRY(hipMemsetAsync(a.hacc, 0, hacc.size() * 8, c->stream));
    {
      ProfScope ps(c, 4);
      if (Hn < kDplSmall) {   // fewer hypotheses than a wave: lane = voxel
        hipLaunchKernelGGL(k_dpl_few, dim3(std::min<unsigned>(dense_blocks((u64)n_r), kDplReduceBlocks)), blk, 0, c->stream, a);
      } else {
        const unsigned n_tiles = (unsigned)((n_r + kDplTile - 1) / kDplTile);
        const unsigned chunks = std::min(n_tiles, std::min<unsigned>(kDplMaxChunks, std::max(1u, 1024u / groups)));
        hipLaunchKernelGGL(k_dpl_score, dim3(groups, chunks), dim3(kDplGroup), 0, c->stream, a);
      }
    }
    ESL_HIP_TRY(hipGetLastError());
    ESL_HIP_TRY(hipMemcpyAsync(hacc.data(), a.hacc, hacc.size() * 8, hipMemcpyDeviceToHost, c->stream));
    ESL_HIP_TRY(hipStreamSynchronize(c->stream));
    // step 5
    int win = -1;
    for (int h = 0; h < Hn; ++h) {
      if (hyp_out) {
        int64_t* ho = hyp_out + ((size_t)r * Hn + h) * 3;
        ho[0] = valid[(size_t)h]; ho[1] = (int64_t)hacc[(size_t)h * 2]; ho[2] = (int64_t)hacc[(size_t)h * 2 + 1];
      }
      if (!valid[(size_t)h]) continue;
      if (win < 0 || dpl_better((long long)hacc[(size_t)h * 2], (long long)hacc[(size_t)h * 2 + 1], h, (long long)hacc[(size_t)win * 2],
                                (long long)hacc[(size_t)win * 2 + 1], win)) win = h;
    }
    const long long win_n = (long long)hacc[(size_t)win * 2], win_s = (long long)hacc[(size_t)win * 2 + 1];
    double fin[4];
    for (int e = 0; e < 4; ++e) fin[e] = planes[(size_t)win * 4 + e];
    long long fin_n = win_n;
    long long mom[kDplMoments];
    // step 6
    int refined = 0;
    if (p.refine) {
      if (dobj_guard(win_n, span)) refined = 3;
      else {
        if (const int rc = dpl_one_pass(c, a, fin, -1, mom)) return rc;
        double re[4];
        dpl_refit(mom, a.kmin, d.p.leaf, re);
        if (const int rc = dpl_one_pass(c, a, re, -1, mom)) return rc;
        if (mom[0] > win_n || (mom[0] == win_n && mom[1] >= win_s)) {
          refined = 1; fin_n = mom[0];
          for (int e = 0; e < 4; ++e) fin[e] = re[e];
        } else {
          refined = 2;
        }
      }
    }
    // step 7
    if (fin_n < p.min_inliers) { stop = 3; break; }
    if (const int rc = dpl_one_pass(c, a, fin, r, mom)) return rc;
    const int q = out->n_planes;   // = r
    double* po = planes_out + 4 * q;
    for (int e = 0; e < 4; ++e) po[e] = fin[e];
    dpl_orient_out(po);
    if (centroid_out) dpl_centroid(mom, a.kmin, d.p.leaf, centroid_out + 3 * q);
    if (stats_out) {
      int32_t* so = stats_out + 8 * q;
      so[0] = (int32_t)mom[0]; so[1] = (int32_t)n_r; so[2] = n_valid; so[3] = win; so[4] = (int32_t)win_n; so[5] = refined; so[6] = 0; so[7] = 0;
    }
    if (samples_out) samples_out[q] = mom[1];
    plane_in.push_back((int32_t)mom[0]);
    out->n_planes = q + 1; out->n_assigned += (int32_t)mom[0];
  }
  out->stop_reason = stop;
  // step 8: every voxel's plane
  if (n_vox_w > 0) {
    {
      ProfScope ps(c, 4);
      hipLaunchKernelGGL(k_dpl_vout, dim3(dense_blocks((u64)n_vox_w)), blk, 0, c->stream, a);
    }
    ESL_HIP_TRY(hipGetLastError());
    ESL_HIP_TRY(hipMemcpyAsync(voxel_plane_out, a.vout, (size_t)n_vox_w * 4, hipMemcpyDeviceToHost, c->stream));
    ESL_HIP_TRY(hipStreamSynchronize(c->stream));
  }
  // step 9
  double uh[3], ground[4];
  if (dpl_up(p.up, uh)) {
    out->ground_index = dpl_ground(planes_out, plane_in.data(), out->n_planes, uh, p.up_min_cos, ground);
    if (ground_out) for (int e = 0; e < 4; ++e) ground_out[e] = ground[e];
  }
  return ESL_OK;
}
