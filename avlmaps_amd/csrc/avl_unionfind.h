// Lock-free union-find on one int32 parent per element, shared by the connected-component labellers (device side).
//
// The invariant: a parent is always a SMALLER index of the same component.  An element starts as its own parent (or below an
// earlier element that is known to belong with it); uf_unite only ever hangs the larger of two roots below the smaller.  So when
// the merging launch ends every component is one tree whose root is its smallest index = its first element, and the result does
// not depend on the order in which the atomics land.  Loads are relaxed at agent scope: a stale parent is still an element of the
// same component with a smaller index, and the walk goes on from there.
#pragma once
#include "avl_common.h"

namespace avl {

__device__ __forceinline__ int uf_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int uf_find(const int* parent, int x) {
    int y = uf_load(parent + x);
    while (y != x) {
        x = y;
        y = uf_load(parent + x);
    }
    return x;
}

__device__ __forceinline__ void uf_unite(int* parent, int a, int b) {
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(parent + a, b);   // a > b: hang a below b if a still is a root
        if (old == a) return;
        a = old;                                    // a had been linked meanwhile: its former parent and b remain to be united
    }
}

// the roots, for avl_scan.h's counting and numbering kernels
struct UfIsRoot {
    const int* parent;
    __device__ __forceinline__ bool operator()(int64_t i) const { return parent[i] == (int)i; }
};

// parent = root, in a launch after the merging one.  A thread walks the whole chain, so one pass is enough however long a chain
// has become.  A negative parent marks an element that takes part in nothing (the islands' background) and is left alone.
// (A template like avl_scan.h's kernels, so that each source that launches it instantiates its own.)
template <int THREADS>
__global__ __launch_bounds__(THREADS) void uf_flatten_kernel(int* __restrict__ parent, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int p = uf_load(parent + i);
        if (p >= 0 && p != (int)i) parent[i] = uf_find(parent, p);
    }
}

}  // namespace avl
