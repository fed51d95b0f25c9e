// Optimistic Adam (Daskalakis et al., "Training GANs with Optimism", Algorithm 1) as a correction pass behind adam_kernel: the player
// steps along 2 d_t - d_{t-1} instead of d_t, d_t = Adam's bias-corrected direction.  adam_kernel has already done p -= lr d_t and
// advanced the step counter; this pass, on the same stream, adds the rest and keeps d_t for the next call:
//
//   d    = (m / bc1) / (sqrt(v) / bc2s + eps)        bc1 = 1 - b1^t, bc2s = sqrt(1 - b2^t), formed in double and rounded to float by
//   p   -= (lr_seg * omega) * (d - prev)             one thread as in adam_kernel, but with t = step[0]: the counter AFTER Adam advanced it
//   prev = d
//
// A streaming pass in adam_kernel's launch shape (256 threads, at most 4096 workgroups, grid-stride loop) with 16-byte accesses:
// 16 B read + 8 B written per parameter.  omega == 0 is the RECORD instantiation: prev = d, p neither read nor written (8 B + 4 B).
// The GUARDED instantiation reads the loss scaler's "last call skipped" word, as ema_kernel does: a skipped Adam step is a skipped
// correction.  Every workgroup also returns while step[0] < 1: no step has been applied, bc1 would be 0 and there is no direction yet.
#include "common.h"

#define OADAM_MAX_SEG 16   // adam.hip's ADAM_MAX_SEG

__device__ __forceinline__ float oadam_direction(float m, float v, float bc1, float bc2s, float eps) {
    return (m / bc1) / (sqrtf(v) / bc2s + eps);
}

template <bool GUARDED, bool RECORD>
__global__ __launch_bounds__(256) void oadam_kernel(float* p, float* __restrict__ prev, const float* m, const float* v, long long n,
                                                    const long long* __restrict__ seg_end, const float* __restrict__ lr, int n_seg,
                                                    float b1, float b2, float eps, float omega, const int32_t* __restrict__ step,
                                                    const int32_t* state) {
    if constexpr (GUARDED) {
        if (state[SC_LAST_OVERFLOW]) return;
    }
    const int t_applied = step[0];   // uniform
    if (t_applied < 1) return;
    __shared__ float s_bc1, s_bc2s;
    __shared__ long long s_end[OADAM_MAX_SEG];
    __shared__ float s_lw[OADAM_MAX_SEG];   // lr_seg * omega
    if (threadIdx.x == 0) {
        const double t = (double)t_applied;
        s_bc1 = (float)(1.0 - pow((double)b1, t));
        s_bc2s = (float)sqrt(1.0 - pow((double)b2, t));
    }
    if (threadIdx.x < n_seg) {
        s_end[threadIdx.x] = seg_end[threadIdx.x];
        s_lw[threadIdx.x] = lr[threadIdx.x] * omega;
    }
    __syncthreads();
    const float bc1 = s_bc1, bc2s = s_bc2s;
    const long long n4 = n >> 2;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const f32x4 mi = ld4(m + 4 * i), vi = ld4(v + 4 * i);
        f32x4 d;
#pragma unroll
        for (int j = 0; j < 4; ++j) d[j] = oadam_direction(mi[j], vi[j], bc1, bc2s, eps);
        if constexpr (!RECORD) {
            const f32x4 old = ld4(prev + 4 * i);
            f32x4 w = ld4(p + 4 * i);
            int sg = 0;   // a segment may end inside the vector: one lookup, then at most n_seg - 1 advances over the four elements
            while (sg < n_seg - 1 && 4 * i >= s_end[sg]) ++sg;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                while (sg < n_seg - 1 && 4 * i + j >= s_end[sg]) ++sg;
                w[j] -= s_lw[sg] * (d[j] - old[j]);
            }
            st4(p + 4 * i, w);
        }
        st4(prev + 4 * i, d);
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {   // the last n % 4 elements
        const long long i = n4 * 4 + threadIdx.x;
        const float d = oadam_direction(m[i], v[i], bc1, bc2s, eps);
        if constexpr (!RECORD) {
            int sg = 0;
            while (sg < n_seg - 1 && i >= s_end[sg]) ++sg;
            p[i] -= s_lw[sg] * (d - prev[i]);
        }
        prev[i] = d;
    }
}

template <bool GUARDED, bool RECORD>
static void oadam_launch(float* p, float* prev, const float* m, const float* v, int64_t n, const int64_t* seg_end, const float* lr,
                         int n_seg, float beta1, float beta2, float eps, float omega, const int32_t* step, const void* scaler_state,
                         void* stream) {
    hipLaunchKernelGGL((oadam_kernel<GUARDED, RECORD>), dim3((int)stream_blocks(n)), dim3(256), 0, (hipStream_t)stream, p, prev, m, v,
                       (long long)n, reinterpret_cast<const long long*>(seg_end), lr, n_seg, beta1, beta2, eps, omega, step,
                       static_cast<const int32_t*>(scaler_state));
}

extern "C" int gim_adam_optimism(float* p, float* prev, const float* m, const float* v, int64_t n, const int64_t* seg_end,
                                 const float* lr, int n_seg, float beta1, float beta2, float eps, float omega, const int32_t* step,
                                 const void* scaler_state, void* stream) {
    GIM_CHECK_ARG(p && prev && m && v && seg_end && lr && step && n > 0, "adam_optimism: bad args");
    GIM_CHECK_ARG(n_seg >= 1 && n_seg <= OADAM_MAX_SEG, "adam_optimism: 1..16 segments");
    GIM_CHECK_ARG(omega >= 0.0f && omega <= 1.0f, "adam_optimism: omega in [0, 1]");   // false for NaN
    GIM_CHECK_ARG(aligned16(p) && aligned16(prev) && aligned16(m) && aligned16(v), "adam_optimism: p, prev, m and v on 16-byte boundaries");
    GIM_CHECK_ARG(!ranges_overlap(prev, p, n) && !ranges_overlap(prev, m, n) && !ranges_overlap(prev, v, n),
                  "adam_optimism: prev must not overlap p, m or v");
    GIM_CHECK_ARG(!((uintptr_t)step & 3) && !((uintptr_t)scaler_state & 3), "adam_optimism: step and scaler_state on 4-byte boundaries");
    const bool record = omega == 0.0f;
    auto launch = scaler_state ? (record ? oadam_launch<true, true> : oadam_launch<true, false>)
                               : (record ? oadam_launch<false, true> : oadam_launch<false, false>);
    launch(p, prev, m, v, n, seg_end, lr, n_seg, beta1, beta2, eps, omega, step, scaler_state, stream);
    return gim_check_launch("gim_adam_optimism");
}
