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
// esl_dense_objects.hip, esl_dense_planes.hip and esl_dense_render.hip work on that sorted list; what they share with this unit, and
// the rule that every kernel of the four keeps, is esl_dense_int.hpp's.
#include "esl_dense_int.hpp"
#include "esl_dense_check.hpp"

#include <rocprim/rocprim.hpp>   // after <cstring>: its headers call memset unqualified

namespace esl {

constexpr int kDenseMaxVoxels = 1 << 26;

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
  if (in) { const DensePixel p = dense_sample_pixel(i, a.stride, a.scols); row = p.row; col = p.col; }
  for (int f = blockIdx.y; f < a.F; f += gridDim.y) {
    const double* P = a.pose + (size_t)f * kDensePose;
    int cat = -1, id = -1;
    u64 key = kDenseEmpty, rgbc = 0;   // sum B | sum G << 16 | sum R << 32 | count << 48: a wave's sums stay below 2^16
    long long s0 = 0, s1 = 0, s2 = 0;
    if (in) {
      const size_t px = ((size_t)f * a.rows + row) * a.cols + col;
      double pc[3], pw[3];
      int k[3];
      // dense_sample_key's three calls, written out: through the helper the four listings change
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

void dense_scratch_stats(const esl_ctx* c, int64_t* allocs, int64_t* bytes) {
  if (!c->dense) return;
  const DenseState& d = *c->dense;
  *allocs = d.set.allocs() + d.obj_set.allocs() + d.pl_set.allocs() + d.rn_set.allocs() + d.al_set.allocs() + d.cv_set.allocs() + d.co_set.allocs();
  *bytes = (int64_t)(d.set.held() + d.obj_set.held() + d.pl_set.held() + d.rn_set.held() + d.al_set.held() + d.cv_set.held() + d.co_set.held());
}

void dense_release(esl_ctx* c) {   // called by esl_ctx_destroy
  if (c->dense) { c->dense->set.release(); c->dense->obj_set.release(); c->dense->pl_set.release(); c->dense->rn_set.release(); c->dense->al_set.release(); c->dense->cv_set.release(); c->dense->co_set.release(); }
  delete c->dense;
  c->dense = nullptr;
}

int dense_list_begin(esl_ctx* c, DenseState& d, DenseList& L) {
  ScratchSet<DB_COUNT>& s = d.set;
  DenseOutArgs& k = L.k;
  const size_t n = (size_t)d.n_voxels;
  std::memset(&k, 0, sizeof(k));
  if (const int rc = s.grow(c, DB_LKEY, n * sizeof(u64))) return rc;
  if (const int rc = s.grow(c, DB_LVAL, n * sizeof(unsigned int))) return rc;
  if (const int rc = s.grow(c, DB_SKEY, n * sizeof(u64))) return rc;
  if (const int rc = s.grow(c, DB_SVAL, n * sizeof(unsigned int))) return rc;
  L.temp_bytes = 0;
  ESL_HIP_TRY(rocprim::radix_sort_pairs(nullptr, L.temp_bytes, s.at<u64>(DB_LKEY), s.at<u64>(DB_SKEY), s.at<unsigned int>(DB_LVAL),
                                        s.at<unsigned int>(DB_SVAL), n, 0, 63, c->stream));
  if (const int rc = s.grow(c, DB_TEMP, L.temp_bytes)) return rc;
  k.keys = s.at<u64>(DB_KEYS); k.rec = s.at<DenseRec>(DB_REC);
  k.H = d.H; k.P = 2 * d.H; k.ctr = s.at<u64>(DB_CTR);
  k.lkey = s.at<u64>(DB_LKEY); k.lval = s.at<unsigned int>(DB_LVAL); k.list_cap = (u64)n;
  k.skey = s.at<u64>(DB_SKEY); k.sval = s.at<unsigned int>(DB_SVAL);
  // k_dense_compact counts from 0.  Nothing between here and the caller's dense_list_launch reads or writes the word: the clear is an
  // independent command on the one stream, wherever among the caller's own clears and uploads it stands
  ESL_HIP_TRY(hipMemsetAsync(k.ctr + DC_LIST, 0, sizeof(u64), c->stream));
  return ESL_OK;
}

int dense_list_launch(esl_ctx* c, DenseState& d, DenseList& L, bool vote, bool gather) {
  ScratchSet<DB_COUNT>& s = d.set;
  DenseOutArgs& k = L.k;
  if (vote) { k.pkeys = s.at<u64>(DB_PKEYS); k.pcnt = s.at<unsigned int>(DB_PCNT); }
  hipLaunchKernelGGL(k_dense_compact, dim3(dense_blocks(k.H)), dim3(kDenseThreads), 0, c->stream, k);
  if (vote) hipLaunchKernelGGL(k_dense_vote, dim3(dense_blocks(k.P)), dim3(kDenseThreads), 0, c->stream, k);
  ESL_HIP_TRY(rocprim::radix_sort_pairs(s.buf[DB_TEMP], L.temp_bytes, s.at<u64>(DB_LKEY), s.at<u64>(DB_SKEY),
                                        s.at<unsigned int>(DB_LVAL), s.at<unsigned int>(DB_SVAL), (size_t)d.n_voxels, 0, 63, c->stream));
  if (gather && k.n_write > 0)   // no caller asks with n_write == 0; an empty grid is no launch
    hipLaunchKernelGGL(k_dense_gather, dim3(dense_blocks((u64)k.n_write)), dim3(kDenseThreads), 0, c->stream, k);
  return ESL_OK;
}

// esl_dense_planes' select (esl_dense_int.hpp).  It stays in this unit: without rocprim::select's device code beside them the
// compiler inlines the shuffles of k_dense_insert<true, *> in another order and their listing changes.
struct DplFree { const int* state; __host__ __device__ bool operator()(int i) const { return state[i] == -2; } };
int dense_select_free(esl_ctx* c, void* tmp, size_t& tmp_bytes, const int* state, int* list, u64* count, size_t n) {
  ESL_HIP_TRY(rocprim::select(tmp, tmp_bytes, rocprim::counting_iterator<int>(0), list, count, n, DplFree{state}, c->stream));
  return ESL_OK;
}

// both tables empty (esl_dense_begin, esl_dense_purge): every key all ones, every record and count zero
static int dense_tables_clear(esl_ctx* c, ScratchSet<DB_COUNT>& s, size_t H, bool pairs) {
  ESL_HIP_TRY(hipMemsetAsync(s.buf[DB_KEYS], 0xFF, H * sizeof(u64), c->stream));
  ESL_HIP_TRY(hipMemsetAsync(s.buf[DB_REC], 0, H * sizeof(DenseRec), c->stream));
  if (pairs) {
    ESL_HIP_TRY(hipMemsetAsync(s.buf[DB_PKEYS], 0xFF, 2 * H * sizeof(u64), c->stream));
    ESL_HIP_TRY(hipMemsetAsync(s.buf[DB_PCNT], 0, 2 * H * sizeof(unsigned int), c->stream));
  }
  return ESL_OK;
}

}  // namespace esl

using namespace esl;

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
  ESL_HIP_TRY(hipMemsetAsync(s.buf[DB_CTR], 0, DC_COUNT * sizeof(u64), c->stream));
  if (with_inst) {
    if (const int rc = s.grow(c, DB_PKEYS, 2 * H * sizeof(u64))) return rc;
    if (const int rc = s.grow(c, DB_PCNT, 2 * H * sizeof(unsigned int))) return rc;
  }
  if (const int rc = dense_tables_clear(c, s, H, with_inst != 0)) return rc;
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
  if (!dense_begun(c, who)) return ESL_ERR_STATE;
  const DenseState& d = *c->dense;
  out->n_samples = d.n_samples;
  out->n_voxels = d.status ? -1 : (int32_t)d.n_voxels;
  out->n_pairs = d.status ? -1 : (int32_t)d.n_pairs;
  out->status = d.status; out->with_color = d.with_color; out->with_inst = d.with_inst; out->pad = 0;
  return ESL_OK;
}

namespace esl {

// step 2 on the host (esl_dense_int.hpp): R and t of every frame, from the given poses or the resident camera states
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

}  // namespace esl

namespace {

// what esl_dense_add_frames, _remove_frames and _move_frames check alike, case by case and in this order; res_cams: the poses (of
// _move_frames: the new ones) are the resident camera states
int dense_frames_check(esl_ctx* c, const char* who, int32_t F, const double K[4], int32_t rows, int32_t cols, const uint16_t* depth,
                       const uint8_t* bgr, const int32_t* inst, bool res_cams) {
  if (!c) return dense_fail(ESL_ERR_INVALID, who, "null ctx");
  if (F < 0) return dense_fail(ESL_ERR_INVALID, who, "negative F");
  if (const char* m = dense_image_check(K, rows, cols)) return dense_fail(ESL_ERR_INVALID, who, m);
  if (F > 0 && !depth) return dense_fail(ESL_ERR_INVALID, who, "null depth");
  const DenseState* d = dense_begun(c, who);
  if (!d) return ESL_ERR_STATE;
  if (F > 0 && d->with_color && !bgr) return dense_fail(ESL_ERR_STATE, who, "null bgr on a map begun with colour");
  if (F > 0 && d->with_inst && !inst) return dense_fail(ESL_ERR_STATE, who, "null inst on a map begun with labels");
  return resident_source_check(c, who, res_cams && F > 0, F, false, 0);
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
    void (*const insert)(DenseArgs) = remove ? (d.combine ? k_dense_insert<true, true> : k_dense_insert<false, true>)
                                             : (d.combine ? k_dense_insert<true, false> : k_dense_insert<false, false>);
    hipLaunchKernelGGL(insert, grid, dim3(kDenseThreads), 0, c->stream, k);
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

// the five counts and the status that both results hold; a removal's result holds two counts more
template <class Result>
void dense_counts(const u64 ctr[DC_COUNT], int status, Result* out) {
  out->n_sampled = (int64_t)ctr[DC_SAMPLED]; out->n_zero = (int64_t)ctr[DC_ZERO]; out->n_depth_out = (int64_t)ctr[DC_DEPTH_OUT];
  out->n_key_out = (int64_t)ctr[DC_KEY_OUT]; out->n_used = (int64_t)ctr[DC_USED]; out->status = status; out->pad = 0;
}
void dense_result(const u64 ctr[DC_COUNT], long long, int status, esl_dense_add_result* out) { dense_counts(ctr, status, out); }
void dense_result(const u64 ctr[DC_COUNT], long long emptied, int status, esl_dense_remove_result* out) {
  dense_counts(ctr, status, out);
  out->n_missing = (int64_t)ctr[DC_MISSING]; out->n_emptied = emptied;
}

void dense_slots_of(const DenseState& d, esl_dense_slots* out) {
  if (d.status) { out->voxel_slots = out->dead_voxels = out->pair_slots = out->dead_pairs = -1; return; }
  out->voxel_slots = d.n_voxels + d.dead_voxels; out->dead_voxels = d.dead_voxels;
  out->pair_slots = d.n_pairs + d.dead_pairs; out->dead_pairs = d.dead_pairs;
}

// esl_dense_add_frames and esl_dense_remove_frames: the same call but for the bound on the samples, the sign of the pass and the result
template <class Result>
int dense_frames_call(esl_ctx* c, const char* who, bool remove, const double* cams, int32_t F, const double K[4], int32_t rows, int32_t cols,
                      const uint16_t* depth, const uint8_t* bgr, const int32_t* inst, Result* out) {
  if (const int rc = dense_frames_check(c, who, F, K, rows, cols, depth, bgr, inst, !cams)) return rc;
  DenseState& d = *c->dense;
  if (out) { std::memset(out, 0, sizeof(*out)); out->status = d.status; }
  if (F == 0 || d.status) return ESL_OK;   // no frame; or an invalid map: nothing more is added or removed until the next esl_dense_begin
  ESL_HIP_TRY(hipSetDevice(c->device));
  // the poses: R and t of every frame on the host, before anything changes
  if (const int rc = dense_frames_poses(c, who, cams, F, d.cams, d.pose)) return rc;
  if ((remove ? 0 : d.n_samples) + dense_per_frame(d, rows, cols) * F >= (1ll << 31))
    return dense_fail(ESL_ERR_INVALID, who, remove ? "more samples than a map holds: 2^31" : "n_samples would reach 2^31");
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
  if (const int rc = dense_pass(c, d, k, remove, ctr)) return rc;
  if (out) dense_result(ctr, d.dead_voxels - dead_before, d.status, out);
  return ESL_OK;
}

}  // namespace

extern "C" int esl_dense_add_frames(esl_ctx* c, const double* cams, int32_t F, const double K[4], int32_t rows, int32_t cols,
                                    const uint16_t* depth, const uint8_t* bgr, const int32_t* inst, esl_dense_add_result* out) {
  return dense_frames_call(c, "esl_dense_add_frames", false, cams, F, K, rows, cols, depth, bgr, inst, out);
}

extern "C" int esl_dense_remove_frames(esl_ctx* c, const double* cams, int32_t F, const double K[4], int32_t rows, int32_t cols,
                                       const uint16_t* depth, const uint8_t* bgr, const int32_t* inst, esl_dense_remove_result* out) {
  return dense_frames_call(c, "esl_dense_remove_frames", true, cams, F, K, rows, cols, depth, bgr, inst, out);
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
  if (out) dense_result(ctr, d.dead_voxels - dead_before, d.status, &out->removed);
  if (d.status) {   // the removal left an inconsistent map: nothing is added
    if (out) out->added.status = d.status;
    return ESL_OK;
  }
  k.pose = pose_new;
  if (const int rc = dense_pass(c, d, k, false, ctr)) return rc;
  if (out) dense_result(ctr, 0, d.status, &out->added);
  return ESL_OK;
}

extern "C" int esl_dense_slots_get(esl_ctx* c, esl_dense_slots* out) {
  const char* who = "esl_dense_slots_get";
  if (!c || !out) return dense_fail(ESL_ERR_INVALID, who, "null pointer");
  if (!dense_begun(c, who)) return ESL_ERR_STATE;
  dense_slots_of(*c->dense, out);
  return ESL_OK;
}

extern "C" int esl_dense_purge(esl_ctx* c, esl_dense_slots* before, esl_dense_slots* after) {
  const char* who = "esl_dense_purge";
  if (!c) return dense_fail(ESL_ERR_INVALID, who, "null ctx");
  if (!dense_begun(c, who)) return ESL_ERR_STATE;
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
    if (const int rc = dense_tables_clear(c, s, H, d.with_inst != 0)) return rc;
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
  if (!dense_begun(c, who)) return ESL_ERR_STATE;
  DenseState& d = *c->dense;
  if (d.status) { *n_voxels = -1; return ESL_OK; }   // over capacity or inconsistent: the map is invalid, nothing is written
  *n_voxels = d.n_voxels;
  const long long n = d.n_voxels, nw = std::min<long long>(n, cap);
  const bool any = key_out || xyz_out || count_out || bgr_out || inst_out || votes_out;
  if (nw == 0 || !any) return ESL_OK;
  ESL_HIP_TRY(hipSetDevice(c->device));
  ScratchSet<DB_COUNT>& s = d.set;
  DenseList L;
  if (const int rc = dense_list_begin(c, d, L)) return rc;
  DenseOutArgs& k = L.k;
  if (key_out) { if (const int rc = s.grow(c, DB_OKEY, (size_t)nw * 3 * sizeof(int32_t))) return rc; k.okey = s.at<int>(DB_OKEY); }
  if (xyz_out) { if (const int rc = s.grow(c, DB_OXYZ, (size_t)nw * 3 * sizeof(double))) return rc; k.oxyz = s.at<double>(DB_OXYZ); }
  if (count_out) { if (const int rc = s.grow(c, DB_OCNT, (size_t)nw * sizeof(int32_t))) return rc; k.ocnt = s.at<int>(DB_OCNT); }
  if (bgr_out) { if (const int rc = s.grow(c, DB_OBGR, (size_t)nw * 3)) return rc; k.obgr = s.at<unsigned char>(DB_OBGR); }
  if (inst_out) { if (const int rc = s.grow(c, DB_OINST, (size_t)nw * sizeof(int32_t))) return rc; k.oinst = s.at<int>(DB_OINST); }
  if (votes_out) { if (const int rc = s.grow(c, DB_OVOTES, (size_t)nw * sizeof(int32_t))) return rc; k.ovotes = s.at<int>(DB_OVOTES); }
  k.n_write = nw; k.with_color = d.with_color;
  const bool vote = d.with_inst && (inst_out || votes_out);
  {
    ProfScope ps(c, 4);
    if (const int rc = dense_list_launch(c, d, L, vote, true)) return rc;
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
