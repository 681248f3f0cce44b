// The fixed summation tree of a row's squared distance  sum_j (x[j] - y[j])^2,  shared by sg2_lpips_pair_dist (ppl.hip)
// and sg2_sqdist_rows_fwd (proj_loss.hip).  Its shape depends on F only -- not on the row, the batch or any address:
//   element j belongs to chunk j / 8192, float4 group k = (j % 8192) / 1024, lane t = (j % 1024) / 4, component i = j % 4.
//   stage 1 (sqdist_chunk_sum: one workgroup of 256 threads per (chunk, row)):
//     a thread keeps four accumulators, one per component i, each a SERIAL RUN of 8 squares (k = 0..7);
//     the four are added as a tree of depth 2, then a wave butterfly (depth 6), then the four waves (depth 2);
//   stage 2 (sqdist_final_sum: one workgroup of 256 threads per row): thread t adds the chunk partials t, t + 256, ...
//     in order -- a SERIAL RUN of ceil(chunks / 256) terms, chunks = ceil(F / 8192) -- then butterfly (6) and waves (2).
//   Longest serial runs: 8, then ceil(ceil(F / 8192) / 256); tree depth 2 + 6 + 2 + 6 + 2 = 18.
// No atomics; elements past F add +0.  VEC (both rows 16-byte aligned, F % 4 == 0) reads float4, otherwise element by
// element on the SAME tree, so the bits do not depend on the alignment either.
#pragma once

#include "sg2_common.h"

namespace sg2 {

constexpr int PPL_THREADS = 256;
constexpr int PPL_SERIAL = 8;                               // float4 groups of a thread per chunk
constexpr int PPL_CHUNK = PPL_THREADS * 4 * PPL_SERIAL;     // 8192 elements
constexpr int PPL_DEPTH = 2 + 6 + 2 + 6 + 2;

__device__ __forceinline__ float ppl_wave_sum(float v) {    // a fixed butterfly: every lane gets the same bits
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Sum over the workgroup's four waves, valid in every thread.  red: 4 floats of LDS.
__device__ __forceinline__ float ppl_block_sum(float v, float* red) {
    v = ppl_wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[2]) + (red[1] + red[3]);
}

__device__ __forceinline__ float ppl_sq(float a, float b) {
    const float d = __fsub_rn(a, b);
    return __fmul_rn(d, d);
}

// Stage 1: the sum of chunk c of the rows r0, r1 (F floats each), valid in every thread of the workgroup.
template <bool VEC>
__device__ __forceinline__ float sqdist_chunk_sum(const float* __restrict__ r0, const float* __restrict__ r1, int64_t F,
                                                  int64_t c, float* red) {
    const int64_t j0 = c * PPL_CHUNK + (int64_t)threadIdx.x * 4;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (VEC) {      // F % 4 == 0: a float4 is inside the row or past its end as a whole
        float4 a[PPL_SERIAL], d[PPL_SERIAL];
#pragma unroll
        for (int k = 0; k < PPL_SERIAL; ++k) {
            const int64_t j = j0 + (int64_t)k * (PPL_THREADS * 4);
            const bool in = j < F;
            a[k] = in ? *(const float4*)(r0 + j) : make_float4(0.f, 0.f, 0.f, 0.f);
            d[k] = in ? *(const float4*)(r1 + j) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int k = 0; k < PPL_SERIAL; ++k) {
            acc[0] = __fadd_rn(acc[0], ppl_sq(a[k].x, d[k].x));
            acc[1] = __fadd_rn(acc[1], ppl_sq(a[k].y, d[k].y));
            acc[2] = __fadd_rn(acc[2], ppl_sq(a[k].z, d[k].z));
            acc[3] = __fadd_rn(acc[3], ppl_sq(a[k].w, d[k].w));
        }
    } else {
#pragma unroll
        for (int k = 0; k < PPL_SERIAL; ++k) {
            const int64_t j = j0 + (int64_t)k * (PPL_THREADS * 4);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const bool in = j + i < F;
                const float x = in ? r0[j + i] : 0.f, y = in ? r1[j + i] : 0.f;
                acc[i] = __fadd_rn(acc[i], ppl_sq(x, y));
            }
        }
    }
    return ppl_block_sum(__fadd_rn(__fadd_rn(acc[0], acc[2]), __fadd_rn(acc[1], acc[3])), red);
}

// Stage 2: the sum of a row's chunk partials, valid in every thread of the workgroup.
__device__ __forceinline__ float sqdist_final_sum(const float* __restrict__ p, int64_t chunks, float* red) {
    float acc = 0.f;
    for (int64_t i = threadIdx.x; i < chunks; i += PPL_THREADS) acc = __fadd_rn(acc, p[i]);
    return ppl_block_sum(acc, red);
}

}  // namespace sg2
