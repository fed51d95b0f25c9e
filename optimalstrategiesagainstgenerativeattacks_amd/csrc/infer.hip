// Pointwise / small-reduction kernels of the baseline authenticators' inference path (baselines.py: the siamese net and ArcFace
// IR-SE of the reference's authentication evaluation).  NHWC fp32, forward only.  All of them are bandwidth-bound: one thread moves
// 16 bytes (4 channels) per access, the channel count is a multiple of 4 and every base pointer is 16-byte aligned (checked by the
// entry points), grids are capped and grid-strided.
#include "common.h"

#define GRID_STRIDE(i, n) for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < (n); i += (long long)gridDim.x * 256)

// ---------------------------------------------------------------- 2x2 max pool (+ ReLU)
__global__ __launch_bounds__(256) void maxpool2_act_kernel(const float* __restrict__ x, float* __restrict__ y, int N, int H, int W, int C4,
                                                           int relu) {
    const int Ho = H >> 1, Wo = W >> 1;
    const long long n_out = (long long)N * Ho * Wo * C4;   // in quads
    const long long row = (long long)W * C4 * 4;
    GRID_STRIDE(i, n_out) {
        const int c = (int)(i % C4);
        long long r = i / C4;
        const int wo = (int)(r % Wo); r /= Wo;
        const int ho = (int)(r % Ho);
        const int n = (int)(r / Ho);
        const float* p = x + ((((long long)n * H + 2 * ho) * W + 2 * wo) * C4 + c) * 4;
        const f32x4 a = ld4(p), b = ld4(p + C4 * 4), d = ld4(p + row), e = ld4(p + row + C4 * 4);
        f32x4 v;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            v[q] = fmaxf(fmaxf(a[q], b[q]), fmaxf(d[q], e[q]));
            if (relu) v[q] = fmaxf(v[q], 0.f);
        }
        st4(y + i * 4, v);
    }
}

extern "C" int gim_maxpool2_act(const float* x, float* y, int N, int H, int W, int C, int relu, void* stream) {
    GIM_CHECK_ARG(x && y && N > 0 && H >= 2 && W >= 2 && !(H & 1) && !(W & 1) && C > 0 && C % 4 == 0, "maxpool2_act: bad args (C % 4 == 0)");
    GIM_CHECK_ARG(aligned16(x) && aligned16(y), "maxpool2_act: pointers must be 16-byte aligned");
    const long long n = (long long)N * (H / 2) * (W / 2) * (C / 4);
    hipLaunchKernelGGL(maxpool2_act_kernel, dim3(blocks256(n)), dim3(256), 0, (hipStream_t)stream, x, y, N, H, W, C / 4, relu);
    return gim_check_launch("gim_maxpool2_act");
}

// ---------------------------------------------------------------- per-channel affine (inference BatchNorm)
__global__ __launch_bounds__(256) void channel_affine_kernel(const float* __restrict__ x, const float* __restrict__ scale,
                                                             const float* __restrict__ shift, float* __restrict__ y, long long n4, int C4) {
    GRID_STRIDE(i, n4) {
        const int c = (int)(i % C4) * 4;
        const f32x4 v = ld4(x + i * 4), s = ld4(scale + c), b = ld4(shift + c);
        f32x4 o;
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = v[q] * s[q] + b[q];
        st4(y + i * 4, o);
    }
}

extern "C" int gim_channel_affine(const float* x, const float* scale, const float* shift, float* y, int64_t rows, int C, void* stream) {
    GIM_CHECK_ARG(x && scale && shift && y && rows > 0 && C > 0 && C % 4 == 0, "channel_affine: bad args (C % 4 == 0)");
    GIM_CHECK_ARG(aligned16(x) && aligned16(y) && aligned16(scale) && aligned16(shift), "channel_affine: pointers must be 16-byte aligned");
    const long long n4 = (long long)rows * (C / 4);
    hipLaunchKernelGGL(channel_affine_kernel, dim3(blocks256(n4)), dim3(256), 0, (hipStream_t)stream, x, scale, shift, y, n4, C / 4);
    return gim_check_launch("gim_channel_affine");
}

// ---------------------------------------------------------------- end of an IR-SE unit
// out = res * sigmoid(gate[n, c]) + shortcut[n, oy * ss, ox * ss, c]; optionally out_bn = out * scale[c] + shift[c]
template <bool BN>
__global__ __launch_bounds__(256) void se_tail_kernel(const float* __restrict__ res, const float* __restrict__ gate,
                                                      const float* __restrict__ shortcut, const float* __restrict__ scale,
                                                      const float* __restrict__ shift, float* __restrict__ out, float* __restrict__ out_bn,
                                                      int N, int Ho, int Wo, int C4, int ss) {
    const long long n4 = (long long)N * Ho * Wo * C4;
    const int Hs = Ho * ss, Ws = Wo * ss;
    GRID_STRIDE(i, n4) {
        const int c = (int)(i % C4);
        long long r = i / C4;
        const int ox = (int)(r % Wo); r /= Wo;
        const int oy = (int)(r % Ho);
        const int n = (int)(r / Ho);
        const f32x4 v = ld4(res + i * 4), g = ld4(gate + ((long long)n * C4 + c) * 4);
        const f32x4 sc = ld4(shortcut + ((((long long)n * Hs + oy * ss) * Ws + ox * ss) * C4 + c) * 4);
        f32x4 o;
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = v[q] * (1.0f / (1.0f + expf(-g[q]))) + sc[q];
        st4(out + i * 4, o);
        if constexpr (BN) {
            const f32x4 s = ld4(scale + c * 4), b = ld4(shift + c * 4);
            f32x4 ob;
#pragma unroll
            for (int q = 0; q < 4; ++q) ob[q] = o[q] * s[q] + b[q];
            st4(out_bn + i * 4, ob);
        }
    }
}

extern "C" int gim_se_tail(const float* res, const float* gate, const float* shortcut, const float* scale, const float* shift, float* out,
                           float* out_bn, int N, int Ho, int Wo, int C, int sstride, void* stream) {
    GIM_CHECK_ARG(res && gate && shortcut && out && N > 0 && Ho > 0 && Wo > 0 && C > 0 && C % 4 == 0, "se_tail: bad args (C % 4 == 0)");
    GIM_CHECK_ARG(sstride == 1 || sstride == 2, "se_tail: sstride must be 1 or 2");
    GIM_CHECK_ARG((out_bn != nullptr) == (scale != nullptr) && (scale != nullptr) == (shift != nullptr), "se_tail: out_bn, scale and shift come together");
    GIM_CHECK_ARG(aligned16(res) && aligned16(gate) && aligned16(shortcut) && aligned16(out) && aligned16(out_bn) && aligned16(scale) &&
                      aligned16(shift), "se_tail: pointers must be 16-byte aligned");
    const long long n4 = (long long)N * Ho * Wo * (C / 4);
    if (out_bn)
        hipLaunchKernelGGL(se_tail_kernel<true>, dim3(blocks256(n4)), dim3(256), 0, (hipStream_t)stream, res, gate, shortcut, scale, shift, out,
                           out_bn, N, Ho, Wo, C / 4, sstride);
    else
        hipLaunchKernelGGL(se_tail_kernel<false>, dim3(blocks256(n4)), dim3(256), 0, (hipStream_t)stream, res, gate, shortcut, scale, shift, out,
                           out_bn, N, Ho, Wo, C / 4, sstride);
    return gim_check_launch("gim_se_tail");
}

// ---------------------------------------------------------------- pair score: -|| a / |a| - b / |b| ||^2 per row
// one wave per row (4 rows per workgroup); two passes over a row that stays in cache: norms, then the distance of the normalised rows
// (the expanded form 2 - 2 <a, b> / (|a| |b|) would cancel for near-identical embeddings)
__global__ __launch_bounds__(256) void pair_score_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out,
                                                         int B, int D4) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= B) return;   // wave-uniform
    const float* pa = a + (long long)row * D4 * 4;
    const float* pb = b + (long long)row * D4 * 4;
    float sa = 0.f, sb = 0.f;
    for (int i = lane; i < D4; i += 64) {
        const f32x4 u = ld4(pa + i * 4), v = ld4(pb + i * 4);
#pragma unroll
        for (int q = 0; q < 4; ++q) { sa += u[q] * u[q]; sb += v[q] * v[q]; }
    }
    const float ia = 1.0f / sqrtf(wave_sum(sa)), ib = 1.0f / sqrtf(wave_sum(sb));
    float d = 0.f;
    for (int i = lane; i < D4; i += 64) {
        const f32x4 u = ld4(pa + i * 4), v = ld4(pb + i * 4);
#pragma unroll
        for (int q = 0; q < 4; ++q) { const float t = u[q] * ia - v[q] * ib; d += t * t; }
    }
    d = wave_sum(d);
    if (lane == 0) out[row] = -d;
}

extern "C" int gim_pair_score(const float* a, const float* b, float* out, int B, int D, void* stream) {
    GIM_CHECK_ARG(a && b && out && B > 0 && D > 0 && D % 4 == 0, "pair_score: bad args (D % 4 == 0)");
    GIM_CHECK_ARG(aligned16(a) && aligned16(b), "pair_score: pointers must be 16-byte aligned");
    hipLaunchKernelGGL(pair_score_kernel, dim3((B + 3) / 4), dim3(256), 0, (hipStream_t)stream, a, b, out, B, D / 4);
    return gim_check_launch("gim_pair_score");
}

// ---------------------------------------------------------------- y = x / |x| per row (one wave per row)
__global__ __launch_bounds__(256) void l2norm_rows_kernel(const float* __restrict__ x, float* __restrict__ y, int B, int D4) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= B) return;   // wave-uniform
    const float* px = x + (long long)row * D4 * 4;
    float s = 0.f;
    for (int i = lane; i < D4; i += 64) {
        const f32x4 u = ld4(px + i * 4);
#pragma unroll
        for (int q = 0; q < 4; ++q) s += u[q] * u[q];
    }
    const float nrm = sqrtf(wave_sum(s));
    for (int i = lane; i < D4; i += 64) {
        f32x4 u = ld4(px + i * 4);
#pragma unroll
        for (int q = 0; q < 4; ++q) u[q] = u[q] / nrm;
        st4(y + ((long long)row * D4 + i) * 4, u);
    }
}

extern "C" int gim_l2norm_rows(const float* x, float* y, int B, int D, void* stream) {
    GIM_CHECK_ARG(x && y && B > 0 && D > 0 && D % 4 == 0, "l2norm_rows: bad args (D % 4 == 0)");
    GIM_CHECK_ARG(aligned16(x) && aligned16(y), "l2norm_rows: pointers must be 16-byte aligned");
    hipLaunchKernelGGL(l2norm_rows_kernel, dim3((B + 3) / 4), dim3(256), 0, (hipStream_t)stream, x, y, B, D / 4);
    return gim_check_launch("gim_l2norm_rows");
}

// ---------------------------------------------------------------- |a - b|
__global__ __launch_bounds__(256) void absdiff_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ y, long long n4) {
    GRID_STRIDE(i, n4) {
        const f32x4 u = ld4(a + i * 4), v = ld4(b + i * 4);
        f32x4 o;
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = fabsf(u[q] - v[q]);
        st4(y + i * 4, o);
    }
}

extern "C" int gim_absdiff(const float* a, const float* b, float* y, int64_t n, void* stream) {
    GIM_CHECK_ARG(a && b && y && n > 0 && n % 4 == 0, "absdiff: bad args (n % 4 == 0)");
    GIM_CHECK_ARG(aligned16(a) && aligned16(b) && aligned16(y), "absdiff: pointers must be 16-byte aligned");
    hipLaunchKernelGGL(absdiff_kernel, dim3(blocks256(n / 4)), dim3(256), 0, (hipStream_t)stream, a, b, y, (long long)(n / 4));
    return gim_check_launch("gim_absdiff");
}
