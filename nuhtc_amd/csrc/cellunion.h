// The lock-free union-find over rows that the per-slide point kernels share (gfx950) -- the clusters (cellcluster.hip: the core points)
// and the minimum spanning forest (cellmst.hip: the two ends of every picked edge); the alpha-shape outline (celloutline.hip) runs it over
// EDGE indices instead: the sides of one triangle.  One forest `parent`, by row, with parent[x] <= x
// always: a root is only ever linked under a SMALLER index and the path halving writes an ancestor with atomicMin, so the smallest row of
// a component is a root for ever and the final root IS that row -- canonical with no further pass.  Nothing here waits on another wave:
// every loop is bounded by the thread's own arithmetic (cellcluster.hip states the argument in full).
#pragma once
#include <hip/hip_runtime.h>

namespace {

__device__ __forceinline__ int cc_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root above core row x as far as this thread can see it, halving the path on the way; every step goes to a smaller row
__device__ __forceinline__ int cc_find(int* parent, int x) {
  int p = cc_load(parent + x);
  while (p != x) {
    const int gp = cc_load(parent + p);
    if (gp != p) atomicMin(parent + x, gp);
    x = p;
    p = gp;
  }
  return x;
}

// one tree for the components of core rows a and b.  max(hi, lo) falls with every failed CAS: the loop ends whatever other threads do
__device__ __forceinline__ void cc_unite(int* parent, int a, int b) {
  int hi = cc_find(parent, a), lo = cc_find(parent, b);
  while (hi != lo) {
    if (hi < lo) { const int t = hi; hi = lo; lo = t; }
    const int old = atomicCAS(parent + hi, hi, lo);
    if (old == hi) return;
    hi = cc_find(parent, old);                           // hi was linked meanwhile: old (< hi) is its parent
    lo = cc_find(parent, lo);
  }
}

// the root of core row x once the hooking is complete
__device__ __forceinline__ int cc_root(const int* __restrict__ parent, int x) {
  for (int p = parent[x]; p != x; p = parent[x]) x = p;
  return x;
}

}  // namespace
