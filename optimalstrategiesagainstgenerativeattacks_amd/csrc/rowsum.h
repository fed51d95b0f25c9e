// The two-stage slab scheme of the baseline-training passes (bn_train.hip, irse_train.hip): a per-channel sum over all rows of an
// NHWC fp32 map without float atomics and without allocation.  Stage 1 gives each workgroup a slab of rows and RS_CB channels -
// RS_CL lanes of 4 channels along the channel axis times RS_HG thread groups along the rows - and writes one partial per channel and
// slab into the caller's `partials`; stage 2 (one small launch) combines the partials of a channel in a fixed order.  Two runs are
// bit-identical.
#pragma once
#include "common.h"

constexpr int RS_MAX_SLABS = 1024;
constexpr int RS_MIN_SLAB_ROWS = 64;
constexpr int RS_CB = 64;             // channels per workgroup of a slab kernel
constexpr int RS_CL = RS_CB / 4;      // lanes along channels (16 bytes each)
constexpr int RS_HG = 256 / RS_CL;    // thread groups along rows

// rows per slab; the slab count is ceil(rows / slab_rows(rows)): no slab is empty
static inline long long slab_rows(long long rows) {
    long long ns = (rows + RS_MIN_SLAB_ROWS - 1) / RS_MIN_SLAB_ROWS;
    if (ns > RS_MAX_SLABS) ns = RS_MAX_SLABS;
    if (ns < 1) ns = 1;
    return (rows + ns - 1) / ns;
}
static inline int slab_count(long long rows) {
    const long long rps = slab_rows(rows);
    return (int)((rows + rps - 1) / rps);
}

// sums of NS quads per thread over the RS_HG thread groups, in group order; valid in the threads of group 0
template <int NS>
__device__ __forceinline__ void group_sum(f32x4 (&s)[NS], float (*red)[RS_HG * RS_CB], int cl, int hg) {
#pragma unroll
    for (int k = 0; k < NS; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) red[k][hg * RS_CB + cl * 4 + e] = s[k][e];
    __syncthreads();
    if (hg == 0) {
#pragma unroll
        for (int k = 0; k < NS; ++k)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float a = 0.f;
                for (int g = 0; g < RS_HG; ++g) a += red[k][g * RS_CB + cl * 4 + e];
                s[k][e] = a;
            }
    }
}
// plain sums: partials [NS][n_slabs][C]
template <int NS>
__device__ __forceinline__ void store_partials(const f32x4 (&s)[NS], float* partials, int n_slabs, int slab, int C, int c) {
#pragma unroll
    for (int k = 0; k < NS; ++k) st4(partials + ((long long)k * n_slabs + slab) * C + c, s[k]);
}

// stage 2 of the plain sums (the kernel is in bn_train.hip): o<k>[c] = sum over slabs of partials[k][slab][c] for k < sums <= 3, in
// a fixed order; a<k> (may be NULL): the total is also ADDED there (a parameter's .grad)
void rowsum_finalize(const float* partials, int n_slabs, int C, int sums, float* o0, float* o1, float* o2, float* a0, float* a1, float* a2,
                     hipStream_t st);

// per-channel parameters of a BatchNorm pass over one channel quad
struct BnChan {
    f32x4 mean, invstd, s, beta, a;   // s = gamma * invstd, a = PReLU slope (PRELU only)
};
template <bool PRELU>
__device__ __forceinline__ BnChan bn_chan(const float* gamma, const float* beta, const float* mean, const float* invstd, const float* slope,
                                          int c) {
    BnChan p;
    p.mean = ld4(mean + c);
    p.invstd = ld4(invstd + c);
    p.s = ld4(gamma + c) * p.invstd;
    p.beta = ld4(beta + c);
    if (PRELU) p.a = ld4(slope + c);
    return p;
}
