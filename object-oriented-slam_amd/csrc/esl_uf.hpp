// esl_uf.hpp — the lock-free union-find walks over a forest in global memory, shared by the single-frame fit's Euclidean clustering
// (esl_fit.hip, cl_union / cl_stats) and the dense map's component labelling (esl_dense_objects.hip, k_dobj_union / k_dobj_roots).
// Linking is by index (the larger root goes under the smaller one, by a CAS on the root's own word), so a component's final root is
// its smallest member.  Device code only.
#pragma once
#include <hip/hip_runtime.h>

namespace esl {

// find with path halving: a node is re-pointed at its grandparent.  Linking by index (larger root under smaller) alone
// grows chains hundreds of hops long inside a 4.5k-point cluster, and every hop is an L2 round trip.  The re-pointing is
// a plain (relaxed atomic) STORE: only roots are ever targets of the linking CAS and a non-root never becomes a root
// again, so the only concurrent writers of parent[i] are other halvings, all of them writing ancestors of i -- and a
// same-address read-modify-write costs ~10 ns of serialisation on this part where a store does not.
__device__ __forceinline__ int uf_find(int* parent, int i) {
  for (;;) {
    const int p = __hip_atomic_load(&parent[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p == i) return i;
    const int gp = __hip_atomic_load(&parent[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (gp == p) return p;
    __hip_atomic_store(&parent[i], gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    i = gp;
  }
}

// The same walk on CACHED loads (workgroup-scope relaxed atomics = plain loads the compiler may not fold): an agent-scope load
// goes past this XCD's L2 to the fabric for every hop (~1 - 2 us, and a find is a chain of them); a cached copy of the forest may be
// stale, but a stale parent is an OLDER ancestor of the same node (roots only ever gain parents, halving only re-points at
// ancestors), so the walk still ends at an ancestor: "same ancestor" proves the two points are joined, and a stale "root" is
// caught by the linking CAS, whose return value is the truth (the union loops continue from it).  Only a union stage may use this --
// the statistics stage of the next kernel needs the real roots.
__device__ __forceinline__ int uf_find_cached(int* parent, int i) {
  for (;;) {
    const int p = __hip_atomic_load(&parent[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (p == i) return i;
    const int gp = __hip_atomic_load(&parent[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (gp == p) return p;
    __hip_atomic_store(&parent[i], gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    i = gp;
  }
}

}  // namespace esl
