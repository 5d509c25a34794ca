// Row machinery of the selection kernels (sample_token_kernel of ff_sample.hip, beam_rows_kernel of ff_beam.hip): one 256-thread workgroup
// owns one row of logits and makes 16 to 32 passes over it, each a count or a sum over the order-preserving integer KEYS of its values.
// A bf16 row of up to kRowStageMax columns is staged ONCE into LDS as 16-bit keys (50258 columns: 98 KiB of the CU's 160 KiB) and every
// pass reads it from there with 16-byte LDS reads; longer bf16 rows and fp32 rows are re-read through L2 every pass.  The workgroup has
// its CU to itself (one wave per SIMD): every loop keeps four loads in flight, nothing else would hide their latency.
// Each kernel keeps its own LDS header (partial sums, `red`, ...) and passes in where the key image starts behind it.
#pragma once
#include <type_traits>

#include "ff_common.h"
#include "ff_internal.h"

namespace ff {

constexpr int kRowStageMax = 65536;           // columns of a staged row (128 KiB of keys)

// order-preserving key of a float: a > b  <=>  key(a) > key(b) for all non-NaN values (-0 is +0).  A bf16 value's key is the top 16 bits.
template <int BITS> FF_DEV unsigned ordered_key(float v) {
    unsigned b = __float_as_uint(v);
    if (b == 0x80000000u) b = 0;
    return ((b >> 31) ? ~b : (b | 0x80000000u)) >> (32 - BITS);
}
template <int BITS> FF_DEV float ordered_value(unsigned k) {
    const unsigned k32 = k << (32 - BITS);
    return __uint_as_float((k32 >> 31) ? (k32 & 0x7FFFFFFFu) : (~k32 & (0xFFFFFFFFu << (32 - BITS))));
}

// f(column, value) for the V elements of a row whose start is only element-aligned, like for_row_vectors of ff_loss.hip (scalar head up to
// the next 16-byte boundary, 16-byte vectors, scalar tail) - but one workgroup has a whole CU to itself here, one wave per SIMD, so
// nothing hides a load's latency unless the wave itself keeps several in flight: four vectors are requested before the first is used.
// The order in which a thread sees its columns is the order of the plain loop.
template <typename T, typename F>
FF_DEV void for_row_vectors4(const T* row, int V, F&& f) {
    constexpr int N = Vec<T>::N;
    int head = (int)(((16u - (unsigned)((unsigned long long)row & 15u)) & 15u) / sizeof(T));
    head = head < V ? head : V;
    const int nvec = (V - head) / N, tail0 = head + nvec * N;
    if ((int)threadIdx.x < head) f((int)threadIdx.x, to_f32(row[threadIdx.x]));
    for (int v = threadIdx.x; v < nvec; v += 1024) {
        typename Vec<T>::raw q[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int vj = v + 256 * j;
            q[j] = *(const typename Vec<T>::raw*)(row + head + (vj < nvec ? vj : v) * N);       // (out of range: the first vector again, unused)
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int vj = v + 256 * j;
            if (vj < nvec) {
#pragma unroll
                for (int e = 0; e < N; e++) f(head + vj * N + e, (float)q[j][e]);
            }
        }
    }
    for (int c = tail0 + threadIdx.x; c < V; c += 256) f(c, to_f32(row[c]));
}

// 256 threads; `red`: 4 words of LDS
FF_DEV int block_sum_int(int v, int* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}
FF_DEV unsigned block_max_uint(unsigned v, unsigned* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned w = (unsigned)__shfl_xor((int)v, o, 64);
        v = v > w ? v : w;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const unsigned a = red[0] > red[1] ? red[0] : red[1], b = red[2] > red[3] ? red[2] : red[3];
    return a > b ? a : b;
}

// One row as its keys.  `sk` (used when STAGED): the key image in LDS, 16-byte aligned, keys of columns [0, 8 ceil(V / 8)).  Contracts:
//  - PADDING.  The image's keys of columns >= V are 0, and the vector loops hand out further keys 0 past the image's end.  0 is also the
//    key of a real value (a negative NaN with every payload bit set), so a key 0 does not say "no column".  Count and mass passes compare
//    against thresholds >= 1 (a bisection candidate has a bit set; sampling's lowest threshold is the key above -inf), which no padding
//    key reaches.  A pass without a threshold has to skip key 0 itself: beam's lse does when STAGED, and such a NaN column is dropped
//    with the padding (a row that holds a NaN has no specified result).
//  - ORDER.  Which thread sees which column, and in which order, is part of the interface: floating-point sums are formed in that order,
//    and equal inputs must give equal bits, launch after launch, eager or replayed.
//  - INLINING.  Every functor passed in must be __attribute__((always_inline)): behind a call its captured counters live in scratch
//    memory, in loops that run 16 to 32 times over the row (tests/test_kernel_resources.py holds both kernels to no scratch).
template <typename T, bool STAGED> struct RowKeys {
    static constexpr int BITS = sizeof(T) == 2 ? 16 : 32;
    const T* row;
    int V;
    unsigned short* sk;
    int c0, c1;                                // this thread's own columns [t C, (t + 1) C) cut to V, C = 8 ceil(ceil(V / 256) / 8)

    FF_DEV RowKeys(const T* row_, int V_, unsigned short* sk_) : row(row_), V(V_), sk(sk_) {
        const int C = ((((V + 255) >> 8) + 7) >> 3) << 3, tid = threadIdx.x;
        c0 = tid * C < V ? tid * C : V;
        c1 = c0 + C < V ? c0 + C : V;
    }

    // f(key) for every column; STAGED also visits the padding keys
    template <typename F> FF_DEV void each(F&& f) const {
        if constexpr (STAGED) {
            const int nvec = (V + 7) >> 3;
            for (int v = threadIdx.x; v < nvec; v += 1024) {                       // four LDS reads in flight; past the end: padding keys
                uint4 q[4];
#pragma unroll
                for (int j = 0; j < 4; j++) q[j] = v + 256 * j < nvec ? *(const uint4*)(sk + (v + 256 * j) * 8) : uint4{0u, 0u, 0u, 0u};
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const unsigned w[4] = {q[j].x, q[j].y, q[j].z, q[j].w};
#pragma unroll
                    for (int e = 0; e < 4; e++) { f(w[e] & 0xFFFFu); f(w[e] >> 16); }
                }
            }
        } else {
            for_row_vectors4(row, V, [&](int, float x) __attribute__((always_inline)) { f(ordered_key<BITS>(x)); });
        }
    }

    // f(column, key) over this thread's own columns in column order; f returns true to stop the walk.  STAGED walks whole 16-byte vectors:
    // behind the thread's last column it goes on into padding keys, with columns that may be >= V.  Those calls all have key 0, so a
    // functor that acts only on keys above a threshold or on a finite value never acts on them, and one that indexes by column must
    // look at the key first.  (A per-column test in here is not free - it doubles the work of the walk, which then costs as much as a
    // whole further pass: measured at 50258 bf16 columns, sampling's launch 142.2 against 137.4 us, beam_step 108.2 against 96.8 us.)
    template <typename F> FF_DEV void own(F&& f) const {
        if constexpr (STAGED) {
            bool stop = false;
            for (int c = c0; c < c1 && !stop; c += 32) {
                uint4 q[4];
#pragma unroll
                for (int j = 0; j < 4; j++) q[j] = c + 8 * j < c1 ? *(const uint4*)(sk + c + 8 * j) : uint4{0u, 0u, 0u, 0u};
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const unsigned w[4] = {q[j].x, q[j].y, q[j].z, q[j].w};
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        if (!stop) stop = f(c + 8 * j + 2 * e, w[e] & 0xFFFFu);
                        if (!stop) stop = f(c + 8 * j + 2 * e + 1, w[e] >> 16);
                    }
                }
            }
        } else {
            for (int c = c0; c < c1; c++)
                if (f(c, ordered_key<BITS>(to_f32(row[c])))) break;
        }
    }

    // STAGED: fills the key image and its padding.  Returns the largest key of the row, known to every thread
    FF_DEV unsigned stage(unsigned* red) const {
        unsigned kmax = 0;
        if constexpr (STAGED) {
            for_row_vectors4(row, V, [&](int c, float x) __attribute__((always_inline)) {
                const unsigned k = ordered_key<BITS>(x);
                sk[c] = (unsigned short)k;
                kmax = k > kmax ? k : kmax;
            });
            for (int c = V + threadIdx.x; c < ((V + 7) & ~7); c += 256) sk[c] = 0;
        } else {
            each([&](unsigned k) __attribute__((always_inline)) { kmax = k > kmax ? k : kmax; });
        }
        return block_max_uint(kmax, red);                                          // (its barriers also publish the key image)
    }

    // the K-th largest key = the largest t with count(key >= t) >= K, one pass per key bit (0 when the row has fewer than K columns)
    FF_DEV unsigned kth_largest(int K, int* red) const {
        unsigned tk = 0;
        for (int bit = BITS - 1; bit >= 0; bit--) {
            const unsigned cand = tk | (1u << bit);
            int n = 0;
            each([&](unsigned k) __attribute__((always_inline)) { n += k >= cand ? 1 : 0; });
            if (block_sum_int(n, red) >= K) tk = cand;
        }
        return tk;
    }
};

// ---- host side ----------------------------------------------------------------------------------------------------------------------
// dynamic LDS of a launch: the kernel's own header, then the key image of a staged row
template <bool STAGED> constexpr size_t row_keys_lds(int header, int V) { return header + (STAGED ? (size_t)((V + 7) / 8) * 16 : 0); }

// beyond 64 KiB of dynamic LDS a kernel has to ask once per device (one table per kernel instantiation)
template <auto KERNEL> int allow_dynamic_lds(int bytes, const char* what) {
    static bool attr_done[64] = {};
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= 64 || !attr_done[dev]) {
        hipError_t e = hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        FF_CHECK(e == hipSuccess, FF_ERR_LAUNCH, "hipFuncSetAttribute(%s lds): %s", what, hipGetErrorString(e));
        if (dev >= 0 && dev < 64) attr_done[dev] = true;
    }
    return FF_OK;
}

// launch(T{}, std::bool_constant<STAGED>{}) with the instantiation for a row of V columns; dtype is FF_DTYPE_BF16 or FF_DTYPE_F32
template <typename L> int row_keys_dispatch(int dtype, int V, L&& launch) {
    if (dtype == FF_DTYPE_BF16) return V <= kRowStageMax ? launch(bf16{}, std::true_type{}) : launch(bf16{}, std::false_type{});
    return launch(float{}, std::false_type{});
}

}  // namespace ff
