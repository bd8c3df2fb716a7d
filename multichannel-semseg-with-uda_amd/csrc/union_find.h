// The lock-free union-find that csrc/refine.hip (regions between boundaries) and csrc/edge.hip (Canny's hysteresis) label connected
// components with.  label[x] is the parent of x; a parent is always an index of the SAME component that is <= x (a root points to
// itself), and every link goes from the larger root to the smaller by an integer atomicMin: the final root of a component is its
// smallest index whatever the schedule -- the canonical id, bit-reproducible.  The global forms use agent-scope atomics for EVERY
// access (other workgroups rewrite label[] meanwhile, and a CU's L1 / another XCD's L2 are not refreshed by their stores); the _lds
// forms do the same inside one workgroup's LDS.  A retry strictly lowers a label, so the loops end, and nobody waits for anybody.
#pragma once
#include <hip/hip_runtime.h>

namespace {

__device__ __forceinline__ int rf_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void rf_store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int rf_min(int* p, int v) { return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// labels only ever decrease and label[x] <= x, so the chase ends at a root whoever writes meanwhile
__device__ __forceinline__ int rf_find(int* label, int x) {
  for (;;) {
    const int p = rf_load(label + x);
    if (p == x) return x;
    x = p;
  }
}

__device__ __forceinline__ void rf_union(int* label, int a, int b) {
  for (;;) {
    a = rf_find(label, a);
    b = rf_find(label, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = rf_min(label + a, b);  // a was a root when read: link it below b
    if (old == a) return;
    a = old;  // somebody linked a first: its component (now below `old`) and b's still have to meet
  }
}

__device__ __forceinline__ int rf_find_lds(int* label, int x) {
  for (;;) {
    const int p = __hip_atomic_load(label + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (p == x) return x;
    x = p;
  }
}

__device__ __forceinline__ void rf_union_lds(int* label, int a, int b) {
  for (;;) {
    a = rf_find_lds(label, a);
    b = rf_find_lds(label, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(label + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (old == a) return;
    a = old;
  }
}

}  // namespace
