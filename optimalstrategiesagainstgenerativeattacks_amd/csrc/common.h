// Shared device/host helpers for libgim_hip (gfx950 / CDNA4 only; wave = 64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/gim_hip.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

extern "C" void gim_set_error(const char* msg);

#define GIM_CHECK_ARG(cond, msg)      \
    do {                              \
        if (!(cond)) {                \
            gim_set_error(msg);       \
            return GIM_E_BADARG;      \
        }                             \
    } while (0)

static inline int gim_check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        char buf[256];
        snprintf(buf, sizeof(buf), "%s: %s", what, hipGetErrorString(e));
        gim_set_error(buf);
        return GIM_E_LAUNCH;
    }
    return GIM_OK;
}

// the loss scaler's device words (layout: gim_hip.h, gim_adam_step_scaled); adam.hip writes them, ema.hip reads the last one
enum ScalerWord { SC_SCALE = 0, SC_INV_SCALE, SC_INTERVAL, SC_CLEAN, SC_OVERFLOW, SC_SKIPPED, SC_MIN_SCALE, SC_LAST_OVERFLOW };
static_assert(SC_LAST_OVERFLOW + 1 == GIM_SCALER_WORDS, "scaler state layout (gim_hip.h)");

static inline int ilog2_exact(int v) {  // returns -1 if v is not a power of two
    if (v <= 0 || (v & (v - 1))) return -1;
    int l = 0;
    while ((1 << l) < v) ++l;
    return l;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Sum over a block of NT threads (a multiple of 64); result valid in every thread. `red` = NT / 64 floats of LDS.  The wave
// partials are added in index order.
template <int NT>
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float tot = red[0];
#pragma unroll
    for (int i = 1; i < NT / 64; ++i) tot += red[i];
    return tot;
}
__device__ __forceinline__ float block_sum_256(float v, float* red) { return block_sum<256>(v, red); }

__device__ __forceinline__ float lrelu_f(float v, float slope) { return v > 0.f ? v : v * slope; }

// 16-byte accesses of the NHWC fp32 passes (bn_train.hip, irse_train.hip, infer.hip): 4 channels per thread, base pointers
// checked by the entry points; capped grid of 256-thread blocks for their grid-strided kernels
__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static inline int blocks256(long long n) {
    const long long b = (n + 255) / 256;
    return (int)(b > 4096 ? 4096 : (b < 1 ? 1 : b));
}

// the streaming passes over flat optimizer buffers (ema.hip, oadam.hip) launch adam.hip's grid: one pass of it covers 4096 * 256 * 4 floats
static inline long long stream_blocks(long long n) {
    long long blocks = (n + 1023) / 1024;
    return blocks > 4096 ? 4096 : blocks;
}

// byte ranges [a, a + 4n) and [b, b + 4n) share an element (a == b included)
static inline bool ranges_overlap(const void* a, const void* b, int64_t n) {
    const uintptr_t ua = (uintptr_t)a, ub = (uintptr_t)b, len = (uintptr_t)n * 4;
    return ua < ub + len && ub < ua + len;
}

// conv_tiny.hip: direct convolution of the 3 -> 3 / 1 -> 1 image layers (3x3, 9x9; plain geometry): one workgroup per
// GIM_TINY_TILE x GIM_TINY_TILE output tile of one image.  gim_tiny_shape is the eligibility test and gim_tiny_grid the launch grid
// of all three directions (the planners in conv_igemm.hip report them); the launchers run eligible shapes only.
constexpr int GIM_TINY_TILE = 16;
bool gim_tiny_shape(const gim_conv_shape* s);
dim3 gim_tiny_grid(const gim_conv_shape* s);
void gim_tiny_fwd(const float* x, const float* w, const float* bias, const float* sigma, const float* res, float* y,
                  const gim_conv_shape* s, hipStream_t st);
void gim_tiny_dgrad(const float* dy, const float* w, const float* sigma, const float* mask_x, float* dx, const gim_conv_shape* s,
                    hipStream_t st);
void gim_tiny_wgrad_acc(const float* dy, const float* x, float* acc, float* bias_acc, const gim_conv_shape* s, hipStream_t st);
