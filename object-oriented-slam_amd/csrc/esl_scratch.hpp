// esl_scratch.hpp — the grow-only device scratch of the map-side calls (esl_reloc / _assoc / _merge / _render / _init .hip) and of three
// context-level buffers, written once.  The rule: a slot is asked for `bytes` before every use; it is left alone while it fits and
// replaced otherwise -- contents are NOT kept, the capacity is exactly the largest request so far.  Every owner keeps a set of its own,
// so a pointer one call left behind is never handed to another.  No kernels here.
// Included by esl_ctx.hpp ahead of esl_ctx, which holds three one-slot sets by value: that is why what reads the context takes it as a
// template parameter (Ctx is always esl_ctx; its members are looked up where the function is used, the struct being complete by then).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

namespace esl {

template <int N>
struct ScratchSet {
  void* buf[N] = {};
  size_t cap[N] = {};       // bytes asked for (the allocation is max(cap, 16))
  long long n_allocs = 0;   // hipMalloc calls so far: unchanged by a warm call (esl_debug_scratch_allocs)

  template <class Ctx>
  int grow(Ctx* c, int k, size_t bytes) {
    if (bytes <= cap[k] && buf[k]) return ESL_OK;
    ESL_HIP_TRY(hipStreamSynchronize(c->stream));   // work in flight may still read the old buffer
    if (buf[k]) (void)hipFree(buf[k]);
    buf[k] = nullptr; cap[k] = 0;                   // a failed hipMalloc leaves the slot empty: the next call tries again
    ESL_HIP_TRY(hipMalloc(&buf[k], std::max<size_t>(bytes, 16)));
    cap[k] = bytes;
    ++n_allocs;
    return ESL_OK;
  }
  template <class T>
  T* at(int k) const { return (T*)buf[k]; }
  size_t held() const {
    size_t s = 0;
    for (size_t b : cap) s += b;
    return s;
  }
  long long allocs() const { return n_allocs; }
  void release() {
    for (int k = 0; k < N; ++k) {
      if (buf[k]) (void)hipFree(buf[k]);
      buf[k] = nullptr; cap[k] = 0;
    }
  }
};
using Scratch = ScratchSet<1>;   // a single buffer: slot 0

// grow slot k, then copy `bytes` (if any) from the host into it on the context's stream; *dev = the slot
template <int N, class Ctx, class T>
int upload(Ctx* c, ScratchSet<N>& s, int k, const T* host_src, size_t bytes, const T** dev) {
  if (const int rc = s.grow(c, k, bytes)) return rc;
  if (bytes) ESL_HIP_TRY(hipMemcpyAsync(s.buf[k], host_src, bytes, hipMemcpyHostToDevice, c->stream));
  *dev = (const T*)s.buf[k];
  return ESL_OK;
}

// "a host array, or NULL = the resident state": upload the former into slot k, or hand back the latter
template <int N, class Ctx, class T>
int source(Ctx* c, ScratchSet<N>& s, int k, const T* host_or_null, const T* resident, size_t bytes, const T** dev) {
  if (host_or_null) return upload(c, s, k, host_or_null, bytes, dev);
  *dev = resident;
  return ESL_OK;
}

// the check that goes with source(): res_cams / res_objs = the call reads the resident cameras / ellipsoids (a NULL array of F / M > 0)
template <class Ctx>
int resident_source_check(Ctx* c, const char* who, bool res_cams, int F, bool res_objs, int M) {
  if (!res_cams && !res_objs) return ESL_OK;
  const std::string w = std::string(who) + ": ";
  if (!c->graph_loaded || !c->states_loaded) {
    set_error(w + "NULL " + (res_cams ? "cams" : "objs") + " needs a resident graph with states");
    return ESL_ERR_STATE;
  }
  if (res_cams && F != c->g.n_cams) { set_error(w + "F differs from the resident graph's n_cams"); return ESL_ERR_INVALID; }
  if (res_objs && M != c->g.n_objs) { set_error(w + "M differs from the resident graph's n_objs"); return ESL_ERR_INVALID; }
  return ESL_OK;
}

}  // namespace esl
