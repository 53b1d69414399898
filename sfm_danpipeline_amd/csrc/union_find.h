// union_find.h -- the no-wait union-find of the device: trees.hip joins the occupied stem cells with it, tracks.hip the
// matched features.  parent[x] <= x and a root is its own parent; roots only move down (atomicMin), so that a set ends at
// its least member whatever the order of the joins.  No spin, no hand-off: every step of a loop lowers a root.
#pragma once
#include <hip/hip_runtime.h>

namespace sfmuf {

__device__ __forceinline__ int root_of(int* parent, int x) {
  for (;;) {  // (parent[x] <= x and a root is its own parent: the walk ends)
    const int up = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (up == x) return x;
    x = up;
  }
}
// joins the sets of a and b: the larger root is hooked under the smaller with atomicMin; when another thread hooked it first,
// that thread's (smaller) target is joined instead.  Every step lowers a root, so the loop ends without waiting for anybody.
__device__ __forceinline__ void unite(int* parent, int a, int b) {
  for (;;) {
    a = root_of(parent, a);
    b = root_of(parent, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(parent + a, b);
    if (old == a) return;
    a = old;
  }
}

}  // namespace sfmuf
