// rocPRIM's stable radix sort of pairs with its temporary storage from the stream's pool, shared by the entry points that sort a
// workspace once per call (the sparse-voxel labeller, avl_pool_rows, avl_object_relations).  The sorts that own their temporary
// storage (avl_heat.hip, avl_finalize.hip, avl_replay.hip, avl_rows.hip, avl_merge.hip, avl_merge2.hip) stay where they are.
#pragma once
#include <rocprim/device/device_radix_sort.hpp>

#include "avl_common.h"

namespace avl {

// n pairs over the low `bits` bits of the keys: size query, hipMallocAsync (of at least 16 bytes), sort, hipFreeAsync
template <typename Key, typename Val>
static int sort_pairs_pooled(const char* who, Key* keys_in, Key* keys_out, Val* vals_in, Val* vals_out, int64_t n, int bits, hipStream_t st) {
    void* tmp = nullptr;
    size_t tmp_bytes = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, tmp_bytes, keys_in, keys_out, vals_in, vals_out, (size_t)n, 0, bits, st);
    if (e == hipSuccess) e = hipMallocAsync(&tmp, tmp_bytes ? tmp_bytes : 16, st);
    if (e == hipSuccess) {
        e = rocprim::radix_sort_pairs(tmp, tmp_bytes, keys_in, keys_out, vals_in, vals_out, (size_t)n, 0, bits, st);
        (void)hipFreeAsync(tmp, st);
    }
    if (e != hipSuccess) {
        set_error("%s: the radix sort failed: %s", who, hipGetErrorString(e));
        return AVL_ERR_HIP;
    }
    return AVL_OK;
}

// the number of low bits that hold every value of 0 .. count - 1, at least 1 and at most `most` (<= 64)
static inline int bits_for(unsigned long long count, int most) {
    int bits = 1;
    while (bits < most && (1ull << bits) < count) ++bits;
    return bits;
}

}  // namespace avl
