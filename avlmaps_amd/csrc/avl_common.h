// Internal helpers shared by the HIP translation units of libavlmaps_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "../../include/avlmaps_hip.h"

namespace avl {

void set_error(const char* fmt, ...);

#define AVL_HIP_CHECK(expr)                                                                      \
    do {                                                                                         \
        hipError_t _e = (expr);                                                                  \
        if (_e != hipSuccess) {                                                                  \
            avl::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return AVL_ERR_HIP;                                                                  \
        }                                                                                        \
    } while (0)

#define AVL_REQUIRE(cond, ...)            \
    do {                                  \
        if (!(cond)) {                    \
            avl::set_error(__VA_ARGS__);  \
            return AVL_ERR_INVALID;       \
        }                                 \
    } while (0)

static inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// number of CUs of the current device (cached)
int num_cus();
// workgroups of 256 threads for a grid-stride kernel over `items`: one thread per item until every CU has 16 workgroups
unsigned stride_blocks(int64_t items);

// Small per-thread, per-device scratch buffer owned by the library (grown on demand, never shrunk): the SYNCHRONOUS entry
// points that return host scalars (avl_argmax_f32, avl_topk_f32) keep their partial results here instead of allocating on
// every call.  Valid until the calling thread's next scratch() call; returns nullptr (and sets the error) on failure.
void* scratch(size_t bytes);
// keep what the device's default stream-ordered pool (hipMallocAsync) has grown to instead of handing it back at every synchronisation
// (HIP's default release threshold is 0: tens of ms per GB to map it again); once per device and thread, cheap afterwards
void keep_mempool_once();
void trim_mempool(uint64_t keep_bytes);   // hipMemPoolTrimTo on the device's default pool

constexpr int kWave = 64;

constexpr size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
// the first 256-aligned address at or after p (entry points whose callers may pass any address; their totals carry the slack)
static inline void* align256_ptr(void* p) { return reinterpret_cast<void*>(align256(reinterpret_cast<uintptr_t>(p))); }

// Lays a workspace out as consecutive 256-aligned pieces.  An entry point's *_work_bytes and its consumer call ONE layout function
// built on this (the size query with a null base), so every piece is written once: the consumer never recomputes an offset or
// derives a size by subtraction.  Slack for a base that the entry point aligns itself is added to total() by the layout function.
struct Carver {
    uintptr_t base;
    size_t used = 0;
    explicit Carver(void* b = nullptr) : base(reinterpret_cast<uintptr_t>(b)) {}
    size_t take(size_t bytes) {                       // the piece's offset
        const size_t at = used;
        used += align256(bytes);
        return at;
    }
    template <typename T>
    T* ptr(size_t bytes) { return reinterpret_cast<T*>(base + take(bytes)); }
    size_t total() const { return used; }
};

}  // namespace avl
