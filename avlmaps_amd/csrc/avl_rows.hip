// Row utilities of the multi-GPU merges (avlmaps_amd/parallel.py, merge2.py): scatter-add and divide rows of float64 partial sums,
// and a stable argsort over the low bits of integer keys.  None of them sees a builder handle.
// Compiled with -ffp-contract=off: the division is finalize_kernel's (avl_finalize.hip).
#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>

#include "avl_common.h"

using namespace avl;

extern "C" {

// dst[d_rows[i] - row0, 0:cols] += src[i, 0:cols]  (float64): folds the contributions one rank received from ONE peer into its
// block of final rows.  A peer holds a voxel at most once, so the rows of a call are distinct: plain read-modify-write, and the
// caller's peer-by-peer order of the calls fixes the summation order (reproducible merges).  Wave per row.
__global__ __launch_bounds__(256) void rows_add_f64_kernel(int64_t n, int cols, const int64_t* __restrict__ rows, int64_t row0, int64_t nrows,
                                                           const double* __restrict__ src, int64_t ld_src, double* __restrict__ dst,
                                                           int64_t ld_dst, int* __restrict__ err_flag) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t i = wave0; i < n; i += nwaves) {
        const int64_t r = rows[i] - row0;
        if (r < 0 || r >= nrows) {
            if (lane == 0 && err_flag) atomicOr(err_flag, 1);
            continue;
        }
        const double* a = src + i * ld_src;
        double* o = dst + r * ld_dst;
        for (int c = lane; c < cols; c += 64) o[c] += a[c];
    }
}

// the same for rows of a few columns (the four [alpha, alpha rgb] sums of a side record): a lane per element, not a wave per row
__global__ __launch_bounds__(256) void rows_add_f64_narrow_kernel(int64_t n, int cols, const int64_t* __restrict__ rows, int64_t row0, int64_t nrows,
                                                                  const double* __restrict__ src, int64_t ld_src, double* __restrict__ dst,
                                                                  int64_t ld_dst, int* __restrict__ err_flag) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n * cols; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = t / cols;
        const int c = (int)(t - i * cols);
        const int64_t r = rows[i] - row0;
        if (r < 0 || r >= nrows) {
            if (c == 0 && err_flag) atomicOr(err_flag, 1);
            continue;
        }
        dst[r * ld_dst + c] += src[i * ld_src + c];
    }
}

static void launch_rows_add(int64_t n, int cols, const int64_t* d_rows, int64_t row0, int64_t nrows, const double* d_src, int64_t ld_src,
                            double* d_dst, int64_t ld_dst, int* flag, hipStream_t st) {
    const int64_t maxb = (int64_t)num_cus() * 16;
    if (cols <= 16) {
        const int64_t blocks = std::min<int64_t>((n * cols + 255) / 256, maxb);
        hipLaunchKernelGGL(rows_add_f64_narrow_kernel, dim3((unsigned)blocks), dim3(256), 0, st, n, cols, d_rows, row0, nrows, d_src, ld_src, d_dst,
                           ld_dst, flag);
    } else {
        const int64_t blocks = std::min<int64_t>((n + 3) / 4, maxb);
        hipLaunchKernelGGL(rows_add_f64_kernel, dim3((unsigned)blocks), dim3(256), 0, st, n, cols, d_rows, row0, nrows, d_src, ld_src, d_dst, ld_dst,
                           flag);
    }
}

int avl_rows_add_f64(int64_t n, int cols, const int64_t* d_rows, int64_t row0, int64_t nrows, const double* d_src, int64_t ld_src,
                     double* d_dst, int64_t ld_dst, void* stream) {
    AVL_REQUIRE(n >= 0 && cols > 0 && nrows >= 0 && ld_src >= cols && ld_dst >= cols, "avl_rows_add_f64: bad shape");
    if (n == 0) return AVL_OK;
    AVL_REQUIRE(d_rows && d_src && d_dst, "avl_rows_add_f64: null pointer");
    hipStream_t st = as_stream(stream);
    int* flag = static_cast<int*>(avl::scratch(64));
    if (!flag) return AVL_ERR_HIP;
    AVL_HIP_CHECK(hipMemsetAsync(flag, 0, sizeof(int), st));
    launch_rows_add(n, cols, d_rows, row0, nrows, d_src, ld_src, d_dst, ld_dst, flag, st);
    int h = 0;
    AVL_HIP_CHECK(hipMemcpyAsync(&h, flag, sizeof(int), hipMemcpyDeviceToHost, st));
    AVL_HIP_CHECK(hipStreamSynchronize(st));
    AVL_REQUIRE(h == 0, "avl_rows_add_f64: a row index lies outside [row0, row0 + nrows)");
    return AVL_OK;
}

int avl_rows_add_f64_async(int64_t n, int cols, const int64_t* d_rows, int64_t row0, int64_t nrows, const double* d_src, int64_t ld_src,
                           double* d_dst, int64_t ld_dst, int32_t* d_err_flag, void* stream) {
    AVL_REQUIRE(n >= 0 && cols > 0 && nrows >= 0 && ld_src >= cols && ld_dst >= cols, "avl_rows_add_f64_async: bad shape");
    if (n == 0) return AVL_OK;
    AVL_REQUIRE(d_rows && d_src && d_dst && d_err_flag, "avl_rows_add_f64_async: null pointer");
    launch_rows_add(n, cols, d_rows, row0, nrows, d_src, ld_src, d_dst, ld_dst, reinterpret_cast<int*>(d_err_flag), as_stream(stream));
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

// out[rows[i], :] = (float)(acc[i, :] / w[rows[i]]): the shared rows of a rank's block from their float64 sums -- finalize_kernel's
// division -- without the (k, D) float64 and float32 temporaries of the tensor expression.  Wave per row.
__global__ __launch_bounds__(256) void rows_div_f32_kernel(int64_t k, int D, const double* __restrict__ acc, const int64_t* __restrict__ rows,
                                                           const double* __restrict__ w4, float* __restrict__ out, int64_t n_out,
                                                           int* __restrict__ err_flag) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t i = wave0; i < k; i += nwaves) {
        const int64_t r = rows[i];
        if (r < 0 || r >= n_out) {
            if (lane == 0 && err_flag) atomicOr(err_flag, 1);
            continue;
        }
        const double w = w4[r * 4];
        const double* a = acc + i * D;
        float* o = out + r * D;
        for (int c = lane; c < D; c += 64) o[c] = (float)(a[c] / w);
    }
}

int avl_rows_div_f32(int64_t k, int D, const double* d_acc, const int64_t* d_rows, const double* d_w4, float* d_out, int64_t n_out,
                     int32_t* d_err_flag, void* stream) {
    AVL_REQUIRE(k >= 0 && D > 0 && n_out >= 0, "avl_rows_div_f32: bad shape");
    if (k == 0) return AVL_OK;
    AVL_REQUIRE(d_acc && d_rows && d_w4 && d_out, "avl_rows_div_f32: null pointer");
    int64_t blocks = (k + 3) / 4;
    const int64_t maxb = (int64_t)num_cus() * 16;
    if (blocks > maxb) blocks = maxb;
    hipLaunchKernelGGL(rows_div_f32_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), k, D, d_acc, d_rows, d_w4, d_out, n_out,
                       reinterpret_cast<int*>(d_err_flag));
    AVL_HIP_CHECK(hipGetLastError());
    return AVL_OK;
}

// values of the sort below: 0, 1, 2, ...
__global__ void iota64_kernel(int64_t* __restrict__ v, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) v[i] = i;
}

}  // extern "C"

template <typename K>
static hipError_t argsort_bits_impl(void* tmp, size_t& tmp_bytes, const void* keys, void* keys_out, const int64_t* iota, int64_t* perm,
                                    int64_t n, int bits, hipStream_t st) {
    // LSD radix sort over the low `bits` bits only (the keys are non-negative and smaller than 2^bits): stable
    return rocprim::radix_sort_pairs(tmp, tmp_bytes, reinterpret_cast<const K*>(keys), reinterpret_cast<K*>(keys_out), iota, perm,
                                     (size_t)n, 0, bits, st);
}

// work buffer of avl_argsort_bits: [values 0..n-1 | sorted keys | rocPRIM's own storage (its size depends on the bit range: rocPRIM
// picks the passes by it)] from the first 256-aligned address on; the total carries 256 bytes of slack for that
struct ArgsortWork { int64_t* iota; void *keys_out, *tmp; size_t tmp_bytes, total; };
static int argsort_layout(int64_t n, int key_bytes, int bits, void* d_work, ArgsortWork& w) {
    size_t t = 0;
    const hipError_t e = key_bytes == 8 ? argsort_bits_impl<uint64_t>(nullptr, t, nullptr, nullptr, nullptr, nullptr, n ? n : 1, bits, nullptr)
                                        : argsort_bits_impl<uint32_t>(nullptr, t, nullptr, nullptr, nullptr, nullptr, n ? n : 1, bits, nullptr);
    AVL_HIP_CHECK(e);
    Carver c(align256_ptr(d_work));
    w.iota = c.ptr<int64_t>((size_t)n * 8);
    w.keys_out = c.ptr<void>((size_t)n * key_bytes);
    w.tmp_bytes = align256(t);
    w.tmp = c.ptr<void>(w.tmp_bytes);
    w.total = c.total() + 256;
    return AVL_OK;
}

extern "C" {

int avl_argsort_bits_work_bytes(int64_t n, int key_bytes, int bits, size_t* h_bytes) {
    AVL_REQUIRE(h_bytes && n >= 0 && n < (1ll << 31) && (key_bytes == 4 || key_bytes == 8) && bits >= 1 && bits <= 8 * key_bytes - 1,
                "avl_argsort_bits_work_bytes: bad arguments");
    ArgsortWork w;
    int rc = argsort_layout(n, key_bytes, bits, nullptr, w);
    if (rc != AVL_OK) return rc;
    *h_bytes = w.total;
    return AVL_OK;
}

int avl_argsort_bits(int64_t n, const void* d_keys, int key_bytes, int bits, int64_t* d_perm, void* d_work, size_t work_bytes,
                     void* stream) {
    AVL_REQUIRE(n >= 0 && n < (1ll << 31), "avl_argsort_bits: bad n");
    AVL_REQUIRE(key_bytes == 4 || key_bytes == 8, "avl_argsort_bits: keys are int32 or int64");
    AVL_REQUIRE(bits >= 1 && bits <= 8 * key_bytes - 1, "avl_argsort_bits: bits must be in [1, %d]", 8 * key_bytes - 1);
    if (n == 0) return AVL_OK;
    AVL_REQUIRE(d_keys && d_perm && d_work, "avl_argsort_bits: null pointer");
    ArgsortWork w;
    int rc = argsort_layout(n, key_bytes, bits, d_work, w);
    if (rc != AVL_OK) return rc;
    AVL_REQUIRE(work_bytes >= w.total, "avl_argsort_bits: work buffer of %zu bytes, %zu needed (avl_argsort_bits_work_bytes)", work_bytes, w.total);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(iota64_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)), dim3(256), 0, st, w.iota, n);
    size_t tmp_bytes = w.tmp_bytes;
    const hipError_t e = key_bytes == 8 ? argsort_bits_impl<uint64_t>(w.tmp, tmp_bytes, d_keys, w.keys_out, w.iota, d_perm, n, bits, st)
                                        : argsort_bits_impl<uint32_t>(w.tmp, tmp_bytes, d_keys, w.keys_out, w.iota, d_perm, n, bits, st);
    if (e != hipSuccess) {
        set_error("avl_argsort_bits: %s", hipGetErrorString(e));
        return AVL_ERR_HIP;
    }
    return AVL_OK;
}

}  // extern "C"
