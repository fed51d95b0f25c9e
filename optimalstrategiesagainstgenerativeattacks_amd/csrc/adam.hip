// Fused multi-tensor Adam over flat parameter / gradient / moment buffers (HBM-bound: 16 B read +
// 12 B written per parameter) plus the library-wide error string.
//
// torch.optim.Adam form (no weight decay, no amsgrad):
//   m = b1*m + (1-b1)*g ; v = b2*v + (1-b2)*g*g
//   p -= (lr / (1-b1^t)) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
// The step counter lives in device memory and is advanced by a 1-thread kernel enqueued after the
// update, so a captured hipGraph replays correctly.
//
// gim_adam_step_scaled: the same update behind a dynamic loss scale whose state is eight words of device memory (layout:
// include/gim_hip.h).  A non-finite test of the gradient bucket sets the overflow word, the GUARDED instantiation of adam_kernel
// returns without touching p, m, v when it is set, and a 1-thread kernel moves scale, counters and the Adam step: no host read.
#include <string.h>

#include "common.h"

static thread_local char g_err[512] = "";
extern "C" void gim_set_error(const char* msg) {
    strncpy(g_err, msg, sizeof(g_err) - 1);
    g_err[sizeof(g_err) - 1] = 0;
}
extern "C" const char* gim_last_error(void) { return g_err; }
extern "C" int gim_version(void) { return 1; }

#define ADAM_MAX_SEG 16

struct AdamSeg {
    long long end[ADAM_MAX_SEG];
};

// GUARDED: `state` = the loss scaler's words; gscale is multiplied by its 1 / scale, and a set overflow word skips the update
template <bool GUARDED>
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, long long n, const long long* __restrict__ seg_end,
                                                   const float* __restrict__ lr, int n_seg, float b1, float b2, float eps,
                                                   float gscale, const int32_t* __restrict__ step, const int32_t* state) {
    __shared__ float s_bc1, s_bc2s;
    __shared__ long long s_end[ADAM_MAX_SEG];
    __shared__ float s_lr[ADAM_MAX_SEG];
    if (threadIdx.x == 0) {
        const double t = (double)(step[0] + 1);
        s_bc1 = (float)(1.0 - pow((double)b1, t));
        s_bc2s = (float)sqrt(1.0 - pow((double)b2, t));
    }
    if (threadIdx.x < n_seg) {
        s_end[threadIdx.x] = seg_end[threadIdx.x];
        s_lr[threadIdx.x] = lr[threadIdx.x];
    }
    if constexpr (GUARDED) {   // one read of the overflow word per workgroup
        __shared__ int s_skip;
        __shared__ float s_inv;
        if (threadIdx.x == 0) {
            s_skip = state[SC_OVERFLOW];
            s_inv = __int_as_float(state[SC_INV_SCALE]);
        }
        __syncthreads();
        if (s_skip) return;
        gscale *= s_inv;
    } else {
        __syncthreads();
    }
    const float bc1 = s_bc1, bc2s = s_bc2s;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        int sg = 0;
        while (sg < n_seg - 1 && i >= s_end[sg]) ++sg;
        const float gr = g[i] * gscale;
        const float mi = b1 * m[i] + (1.0f - b1) * gr;
        const float vi = b2 * v[i] + (1.0f - b2) * gr * gr;
        m[i] = mi;
        v[i] = vi;
        const float denom = sqrtf(vi) / bc2s + eps;
        p[i] -= (s_lr[sg] / bc1) * (mi / denom);
    }
}

__global__ void adam_advance_kernel(int32_t* step) { step[0] += 1; }

// inf or NaN anywhere in g[0 .. n) -> overflow word: exponent bits all ones, per lane; at most one atomic per wave, and only on overflow
__global__ __launch_bounds__(256) void grad_nonfinite_kernel(const float* __restrict__ g, long long n, int32_t* state) {
    const long long n4 = n >> 2;
    const uint4* g4 = reinterpret_cast<const uint4*>(g);
    bool bad = false;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const uint4 q = g4[i];
        bad |= (q.x & 0x7F800000u) == 0x7F800000u || (q.y & 0x7F800000u) == 0x7F800000u || (q.z & 0x7F800000u) == 0x7F800000u ||
               (q.w & 0x7F800000u) == 0x7F800000u;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3))   // the last n % 4 elements
        bad |= (__float_as_uint(g[n4 * 4 + threadIdx.x]) & 0x7F800000u) == 0x7F800000u;
    if (__ballot(bad) != 0 && (threadIdx.x & 63) == 0) atomicOr(&state[SC_OVERFLOW], 1);
}

// replaces adam_advance_kernel behind the guarded update: growth 2 and backoff 1/2 only, so scale and 1 / scale stay exact
__global__ void scaler_update_kernel(int32_t* step, int32_t* state) {
    float scale = __int_as_float(state[SC_SCALE]);
    const int overflow = state[SC_OVERFLOW] != 0;
    if (overflow) {
        scale = fmaxf(scale * 0.5f, __int_as_float(state[SC_MIN_SCALE]));
        state[SC_CLEAN] = 0;
        state[SC_SKIPPED] += 1;
    } else {
        step[0] += 1;
        int clean = state[SC_CLEAN] + 1;
        if (clean >= state[SC_INTERVAL]) {
            scale *= 2.0f;
            clean = 0;
        }
        state[SC_CLEAN] = clean;
    }
    state[SC_SCALE] = __float_as_int(scale);
    state[SC_INV_SCALE] = __float_as_int(1.0f / scale);
    state[SC_LAST_OVERFLOW] = overflow;
    state[SC_OVERFLOW] = 0;
}

extern "C" int gim_adam_step(float* p, const float* g, float* m, float* v, int64_t n, const int64_t* seg_end, const float* lr,
                             int n_seg, float beta1, float beta2, float eps, float grad_scale, int32_t* step, void* stream) {
    GIM_CHECK_ARG(p && g && m && v && seg_end && lr && step && n > 0, "adam_step: bad args");
    GIM_CHECK_ARG(n_seg >= 1 && n_seg <= ADAM_MAX_SEG, "adam_step: 1..16 segments");
    long long blocks = (n + 1023) / 1024;
    if (blocks > 4096) blocks = 4096;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(adam_kernel<false>, dim3((int)blocks), dim3(256), 0, st, p, g, m, v, (long long)n,
                       reinterpret_cast<const long long*>(seg_end), lr, n_seg, beta1, beta2, eps, grad_scale, step, nullptr);
    hipLaunchKernelGGL(adam_advance_kernel, dim3(1), dim3(1), 0, st, step);
    return gim_check_launch("gim_adam_step");
}

extern "C" int gim_adam_step_scaled(float* p, const float* g, float* m, float* v, int64_t n, const int64_t* seg_end, const float* lr,
                                    int n_seg, float beta1, float beta2, float eps, float grad_scale, int32_t* step, void* state,
                                    void* stream) {
    GIM_CHECK_ARG(p && g && m && v && seg_end && lr && step && state && n > 0, "adam_step_scaled: bad args");
    GIM_CHECK_ARG(n_seg >= 1 && n_seg <= ADAM_MAX_SEG, "adam_step_scaled: 1..16 segments");
    GIM_CHECK_ARG(!((uintptr_t)g & 15) && !((uintptr_t)state & 3), "adam_step_scaled: g on a 16-byte boundary, state on a 4-byte one");
    long long blocks = (n + 1023) / 1024;
    if (blocks > 4096) blocks = 4096;
    hipStream_t st = (hipStream_t)stream;
    int32_t* sw = static_cast<int32_t*>(state);
    hipLaunchKernelGGL(grad_nonfinite_kernel, dim3((int)blocks), dim3(256), 0, st, g, (long long)n, sw);
    hipLaunchKernelGGL(adam_kernel<true>, dim3((int)blocks), dim3(256), 0, st, p, g, m, v, (long long)n,
                       reinterpret_cast<const long long*>(seg_end), lr, n_seg, beta1, beta2, eps, grad_scale, step, sw);
    hipLaunchKernelGGL(scaler_update_kernel, dim3(1), dim3(1), 0, st, step, sw);
    return gim_check_launch("gim_adam_step_scaled");
}
