// Averaged agents: exponential moving average of a flat parameter buffer, and the in-place exchange of two flat buffers
// (training/utils.py:96-101, accumulate).  Both are streaming passes in adam_kernel's launch shape (256 threads, at most 4096
// workgroups, grid-stride loop) with 16-byte accesses: 8 B read + 4 B written per parameter for the average, 8 + 8 for the exchange.
//
//   gim_ema_update     : avg = decay * avg + (1 - decay) * p, fp32, 1 - decay formed once on the host in fp32.  Behind
//                        gim_adam_step_scaled the GUARDED instantiation reads the scaler's "last call skipped" word and returns
//                        without touching avg when it is set: a skipped optimizer step is a skipped average step, no host read.
//   gim_buffer_exchange: a <-> b as bit patterns (uint4), so NaN payloads and -0 survive; twice is the identity.
#include "common.h"

// GUARDED: `state` = the loss scaler's words after scaler_update_kernel; the read is uniform, one scalar load per wave
template <bool GUARDED>
__global__ __launch_bounds__(256) void ema_kernel(float* __restrict__ avg, const float* __restrict__ p, long long n, float decay,
                                                  float one_minus, const int32_t* state) {
    if constexpr (GUARDED) {
        if (state[SC_LAST_OVERFLOW]) return;
    }
    const long long n4 = n >> 2;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const f32x4 a = ld4(avg + 4 * i), w = ld4(p + 4 * i);
        st4(avg + 4 * i, decay * a + one_minus * w);
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {   // the last n % 4 elements
        const long long i = n4 * 4 + threadIdx.x;
        avg[i] = decay * avg[i] + one_minus * p[i];
    }
}

__global__ __launch_bounds__(256) void exchange_kernel(uint32_t* __restrict__ a, uint32_t* __restrict__ b, long long n) {
    const long long n4 = n >> 2;
    uint4* a4 = reinterpret_cast<uint4*>(a);
    uint4* b4 = reinterpret_cast<uint4*>(b);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const uint4 qa = a4[i], qb = b4[i];
        a4[i] = qb;
        b4[i] = qa;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const long long i = n4 * 4 + threadIdx.x;
        const uint32_t wa = a[i], wb = b[i];
        a[i] = wb;
        b[i] = wa;
    }
}

extern "C" int gim_ema_update(float* avg, const float* p, int64_t n, float decay, const void* scaler_state, void* stream) {
    GIM_CHECK_ARG(avg && p && n > 0, "ema_update: bad args");
    GIM_CHECK_ARG(decay >= 0.0f && decay < 1.0f, "ema_update: decay in [0, 1)");   // false for NaN
    GIM_CHECK_ARG(aligned16(avg) && aligned16(p), "ema_update: avg and p on 16-byte boundaries");
    GIM_CHECK_ARG(!ranges_overlap(avg, p, n), "ema_update: avg and p must not overlap");
    GIM_CHECK_ARG(!((uintptr_t)scaler_state & 3), "ema_update: scaler_state on a 4-byte boundary");
    const float one_minus = 1.0f - decay;
    const dim3 grid((int)stream_blocks(n));
    hipStream_t st = (hipStream_t)stream;
    if (scaler_state)
        hipLaunchKernelGGL(ema_kernel<true>, grid, dim3(256), 0, st, avg, p, (long long)n, decay, one_minus,
                           static_cast<const int32_t*>(scaler_state));
    else
        hipLaunchKernelGGL(ema_kernel<false>, grid, dim3(256), 0, st, avg, p, (long long)n, decay, one_minus, nullptr);
    return gim_check_launch("gim_ema_update");
}

extern "C" int gim_buffer_exchange(float* a, float* b, int64_t n, void* stream) {
    GIM_CHECK_ARG(a && b && n > 0, "buffer_exchange: bad args");
    GIM_CHECK_ARG(aligned16(a) && aligned16(b), "buffer_exchange: a and b on 16-byte boundaries");
    GIM_CHECK_ARG(!ranges_overlap(a, b, n), "buffer_exchange: a and b must not overlap");
    hipLaunchKernelGGL(exchange_kernel, dim3((int)stream_blocks(n)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<uint32_t*>(a), reinterpret_cast<uint32_t*>(b), (long long)n);
    return gim_check_launch("gim_buffer_exchange");
}
