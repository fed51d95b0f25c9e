// Training passes of the ArcFace baseline on the IR-SE backbone (baseline_training.py; arcface/models.py:16-84,120-208) beyond the
// convolutions: BatchNorm with BATCH statistics (not fused with a pool; optionally with the per-channel PReLU behind it), PReLU,
// the backward of the SE tail, the even-position subsample, dropout from a counter hash, and the margin head (row / column l2
// normalisation, additive angular margin, softmax cross-entropy).  Every pass is bandwidth-bound.
//
// Maps are NHWC fp32 with C % 4 == 0 and 16-byte aligned base pointers (checked by the entry points): one thread moves 16 bytes
// (4 channels) per access, lanes run along the channel axis.  The head's matrices are [rows][cols] with any column count (scalar).
//
// No float atomics and no allocation.  A sum over the rows of a map follows the two-stage slab scheme of rowsum.h: stage 1 gives
// each workgroup a slab of rows (gim_bn_slabs(rows) slabs) and writes one partial per channel into the caller's `partials`
// ([3][slabs][C] floats), stage 2 (rowsum_finalize) adds the partials of a channel in a fixed order.  Two runs are bit-identical.
#include "rowsum.h"

// ---------------------------------------------------------------- BatchNorm with batch statistics (+ PReLU)
template <bool PRELU>
__global__ __launch_bounds__(256) void bn_apply_fwd_kernel(const float* __restrict__ z, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, const float* __restrict__ mean,
                                                           const float* __restrict__ invstd, const float* __restrict__ slope,
                                                           float* __restrict__ y, long long n4, int C4) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % C4) * 4;
        const BnChan p = bn_chan<PRELU>(gamma, beta, mean, invstd, slope, c);
        const f32x4 v = ld4(z + i * 4);
        f32x4 o;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            o[q] = fmaf(v[q] - p.mean[q], p.s[q], p.beta[q]);
            if (PRELU) o[q] = o[q] > 0.f ? o[q] : o[q] * p.a[q];
        }
        st4(y + i * 4, o);
    }
}

// stage 1 of (sum dyhat, sum dyhat * xhat[, sum_{yhat <= 0} dy * yhat]); dyhat = dy through the PReLU (x > 0 ? 1 : a: torch's rule)
template <bool PRELU>
__global__ __launch_bounds__(256) void bn_bwd_slab_kernel(const float* __restrict__ dy, const float* __restrict__ z,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          const float* __restrict__ mean, const float* __restrict__ invstd,
                                                          const float* __restrict__ slope, float* __restrict__ partials, long long M, int C,
                                                          long long rps, int n_slabs) {
    __shared__ float red[3][RS_HG * RS_CB];
    const int cl = threadIdx.x % RS_CL, hg = threadIdx.x / RS_CL;
    const int c = blockIdx.x * RS_CB + cl * 4;
    const long long r0 = (long long)blockIdx.y * rps;
    const long long r1 = (r0 + rps < M) ? r0 + rps : M;
    const bool ok = c < C;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 s[3] = {zero, zero, zero};
    if (ok) {
        const BnChan p = bn_chan<PRELU>(gamma, beta, mean, invstd, slope, c);
#pragma unroll 4
        for (long long r = r0 + hg; r < r1; r += RS_HG) {
            const f32x4 g = ld4(dy + r * C + c), v = ld4(z + r * C + c);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float xc = v[q] - p.mean[q];
                float d = g[q];
                if (PRELU) {
                    const float yh = fmaf(xc, p.s[q], p.beta[q]);
                    if (!(yh > 0.f)) {
                        s[2][q] += g[q] * yh;
                        d = g[q] * p.a[q];
                    }
                }
                s[0][q] += d;
                s[1][q] += d * (xc * p.invstd[q]);
            }
        }
    }
    group_sum<3>(s, red, cl, hg);
    if (ok && hg == 0) store_partials<3>(s, partials, n_slabs, blockIdx.y, C, c);
}

// dz = gamma * invstd * (dyhat - dbeta / M - xhat * dgamma / M)
template <bool PRELU>
__global__ __launch_bounds__(256) void bn_bwd_dx_kernel(const float* __restrict__ dy, const float* __restrict__ z,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        const float* __restrict__ mean, const float* __restrict__ invstd,
                                                        const float* __restrict__ slope, const float* __restrict__ dgamma,
                                                        const float* __restrict__ dbeta, float* __restrict__ dz, long long n4, int C4,
                                                        float inv_m) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % C4) * 4;
        const BnChan p = bn_chan<PRELU>(gamma, beta, mean, invstd, slope, c);
        const f32x4 mb = ld4(dbeta + c) * inv_m, mg = ld4(dgamma + c) * inv_m;
        const f32x4 g = ld4(dy + i * 4), v = ld4(z + i * 4);
        f32x4 o;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float xc = v[q] - p.mean[q];
            float d = g[q];
            if (PRELU) d = fmaf(xc, p.s[q], p.beta[q]) > 0.f ? d : d * p.a[q];
            o[q] = p.s[q] * (d - mb[q] - xc * p.invstd[q] * mg[q]);
        }
        st4(dz + i * 4, o);
    }
}

// ---------------------------------------------------------------- PReLU (slope == NULL: ReLU)
template <bool SLOPE>
__global__ __launch_bounds__(256) void prelu_fwd_kernel(const float* __restrict__ x, const float* __restrict__ slope, float* __restrict__ y,
                                                        long long n4, int C4) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const f32x4 v = ld4(x + i * 4);
        f32x4 a = {0.f, 0.f, 0.f, 0.f}, o;
        if (SLOPE) a = ld4(slope + (int)(i % C4) * 4);
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = v[q] > 0.f ? v[q] : v[q] * a[q];
        st4(y + i * 4, o);
    }
}

// dx = dy * (x > 0 ? 1 : a) and stage 1 of da = sum_{x <= 0} dy * x, in one pass over a slab of rows
template <bool SLOPE>
__global__ __launch_bounds__(256) void prelu_bwd_slab_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                             const float* __restrict__ slope, float* __restrict__ dx,
                                                             float* __restrict__ partials, long long M, int C, long long rps, int n_slabs) {
    __shared__ float red[1][RS_HG * RS_CB];
    const int cl = threadIdx.x % RS_CL, hg = threadIdx.x / RS_CL;
    const int c = blockIdx.x * RS_CB + cl * 4;
    const long long r0 = (long long)blockIdx.y * rps;
    const long long r1 = (r0 + rps < M) ? r0 + rps : M;
    const bool ok = c < C;
    f32x4 s[1] = {{0.f, 0.f, 0.f, 0.f}};
    if (ok) {
        f32x4 a = {0.f, 0.f, 0.f, 0.f};
        if (SLOPE) a = ld4(slope + c);
#pragma unroll 4
        for (long long r = r0 + hg; r < r1; r += RS_HG) {
            const f32x4 g = ld4(dy + r * C + c), v = ld4(x + r * C + c);
            f32x4 o;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const bool pos = v[q] > 0.f;
                o[q] = pos ? g[q] : g[q] * a[q];
                if (SLOPE) s[0][q] += pos ? 0.f : g[q] * v[q];
            }
            st4(dx + r * C + c, o);
        }
    }
    if (!SLOPE) return;
    group_sum<1>(s, red, cl, hg);
    if (ok && hg == 0) store_partials<1>(s, partials, n_slabs, blockIdx.y, C, c);
}

// ---------------------------------------------------------------- backward of out = res * sigmoid(gate[n, c]) + shortcut
// one workgroup per (image, block of 64 channels) walks the image's pixels: dres = dout * sig, dgate = sig (1 - sig) sum dout * res
__global__ __launch_bounds__(256) void se_tail_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ res,
                                                          const float* __restrict__ gate, float* __restrict__ dres,
                                                          float* __restrict__ dgate, int P, int C) {
    __shared__ float red[1][RS_HG * RS_CB];
    const int cl = threadIdx.x % RS_CL, hg = threadIdx.x / RS_CL;
    const int c = blockIdx.x * RS_CB + cl * 4;
    const long long n = blockIdx.y;
    const bool ok = c < C;
    f32x4 s[1] = {{0.f, 0.f, 0.f, 0.f}};
    f32x4 sig = {0.f, 0.f, 0.f, 0.f};
    if (ok) {
        const f32x4 g = ld4(gate + n * C + c);
#pragma unroll
        for (int q = 0; q < 4; ++q) sig[q] = 1.0f / (1.0f + expf(-g[q]));
        const long long base = n * P * C + c;
#pragma unroll 4
        for (int p = hg; p < P; p += RS_HG) {
            const f32x4 d = ld4(dout + base + (long long)p * C), r = ld4(res + base + (long long)p * C);
            s[0] += d * r;
            st4(dres + base + (long long)p * C, d * sig);
        }
    }
    group_sum<1>(s, red, cl, hg);
    if (ok && hg == 0) st4(dgate + n * C + c, s[0] * sig * (1.0f - sig));
}

// ---------------------------------------------------------------- y[n, i, j] = x[n, 2 i, 2 j] and its transpose
__global__ __launch_bounds__(256) void subsample2_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, long long n4, int Ho, int Wo,
                                                             int C4) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % C4);
        long long r = i / C4;
        const int ox = (int)(r % Wo);
        r /= Wo;
        const int oy = (int)(r % Ho);
        const long long n = r / Ho;
        st4(y + i * 4, ld4(x + ((((n * Ho + oy) * 2) * (2 * Wo) + 2 * ox) * C4 + c) * 4));
    }
}
// every element of dx is written exactly once: dy at the even positions, zero elsewhere
__global__ __launch_bounds__(256) void subsample2_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, long long n4, int H, int W,
                                                             int C4) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % C4);
        long long r = i / C4;
        const int ix = (int)(r % W);
        r /= W;
        const int iy = (int)(r % H);
        const long long n = r / H;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (!((ix | iy) & 1)) v = ld4(dy + (((n * (H / 2) + iy / 2) * (W / 2) + ix / 2) * C4 + c) * 4);
        st4(dx + i * 4, v);
    }
}

// ---------------------------------------------------------------- dropout: keep = hash(seed, offset + element) >= p, in registers
__device__ __forceinline__ uint32_t ir_mix(uint32_t h) {      // the 32-bit finalizer of MurmurHash3
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}
__device__ __forceinline__ float ir_uniform(uint64_t seed, uint64_t ctr) {      // [0, 1) on a 24-bit grid
    uint32_t h = ir_mix((uint32_t)ctr ^ 0x9E3779B9u);
    h = ir_mix(h ^ (uint32_t)(ctr >> 32));
    h = ir_mix(h ^ (uint32_t)seed);
    h = ir_mix(h ^ (uint32_t)(seed >> 32));
    return (float)(h >> 8) * (1.0f / 16777216.0f);
}
__global__ __launch_bounds__(256) void dropout_kernel(const float* __restrict__ x, float* __restrict__ y, long long n4, float p, float scale,
                                                      uint64_t seed, uint64_t offset) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const f32x4 v = ld4(x + i * 4);
        f32x4 o;
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = ir_uniform(seed, offset + (uint64_t)(i * 4 + q)) >= p ? v[q] * scale : 0.f;
        st4(y + i * 4, o);
    }
}

// ---------------------------------------------------------------- backward of y = x / |x| per row (one wave per row)
__global__ __launch_bounds__(256) void l2norm_rows_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                              float* __restrict__ dx, int B, int D4) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= B) return;   // wave-uniform
    const float* px = x + (long long)row * D4 * 4;
    const float* pg = dy + (long long)row * D4 * 4;
    float ss = 0.f, sg = 0.f;
    for (int i = lane; i < D4; i += 64) {
        const f32x4 u = ld4(px + i * 4), g = ld4(pg + i * 4);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            ss += u[q] * u[q];
            sg += u[q] * g[q];
        }
    }
    ss = wave_sum(ss);
    sg = wave_sum(sg);
    const float inv = 1.0f / sqrtf(ss), t = sg / ss;      // dx = (dy - x * <dy, x> / |x|^2) / |x|
    for (int i = lane; i < D4; i += 64) {
        const f32x4 u = ld4(px + i * 4), g = ld4(pg + i * 4);
        st4(dx + ((long long)row * D4 + i) * 4, (g - u * t) * inv);
    }
}

// ---------------------------------------------------------------- l2 normalisation over the ROWS of k [E][N] (one thread per column)
__global__ __launch_bounds__(256) void col_l2norm_fwd_kernel(const float* __restrict__ k, float* __restrict__ out, int E, int N) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= N) return;
    float ss = 0.f;
    for (int e = 0; e < E; ++e) {
        const float v = k[(long long)e * N + j];
        ss += v * v;
    }
    const float nrm = sqrtf(ss);
    for (int e = 0; e < E; ++e) out[(long long)e * N + j] = k[(long long)e * N + j] / nrm;
}
// dk = (dn - n * sum_rows dn * n) / |k|
__global__ __launch_bounds__(256) void col_l2norm_bwd_kernel(const float* __restrict__ dn, const float* __restrict__ k, float* __restrict__ dk,
                                                             int E, int N) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= N) return;
    float ss = 0.f, sg = 0.f;
    for (int e = 0; e < E; ++e) {
        const float v = k[(long long)e * N + j];
        ss += v * v;
        sg += v * dn[(long long)e * N + j];
    }
    const float inv = 1.0f / sqrtf(ss), t = sg / ss;
    for (int e = 0; e < E; ++e) dk[(long long)e * N + j] = (dn[(long long)e * N + j] - k[(long long)e * N + j] * t) * inv;
}

// ---------------------------------------------------------------- additive angular margin on a [B][N] cosine matrix
struct IrMargin {
    float s, cos_m, sin_m, mm, threshold;
};
__global__ __launch_bounds__(256) void arc_margin_fwd_kernel(const float* __restrict__ cosv, const int64_t* __restrict__ label,
                                                             float* __restrict__ out, long long n, int N, IrMargin m) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const long long b = i / N;
        const float c = fminf(fmaxf(cosv[i], -1.0f), 1.0f);
        float v = c;
        if (label[b] == i - b * N) v = (c - m.threshold <= 0.f) ? c - m.mm : c * m.cos_m - sqrtf(1.0f - c * c) * m.sin_m;
        out[i] = v * m.s;
    }
}
__global__ __launch_bounds__(256) void arc_margin_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ cosv,
                                                             const int64_t* __restrict__ label, float* __restrict__ dcos, long long n, int N,
                                                             IrMargin m) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const long long b = i / N;
        const float raw = cosv[i];
        float g = 0.f;
        if (raw >= -1.0f && raw <= 1.0f) {      // the clamp passes the gradient on its closed interval
            g = dout[i] * m.s;
            if (label[b] == i - b * N && !(raw - m.threshold <= 0.f)) g *= m.cos_m + m.sin_m * raw / sqrtf(1.0f - raw * raw);
        }
        dcos[i] = g;
    }
}

// ---------------------------------------------------------------- softmax cross-entropy, one workgroup per row
__global__ __launch_bounds__(256) void softmax_ce_fwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ label,
                                                             float* __restrict__ loss, float* __restrict__ correct, float* __restrict__ lse,
                                                             int N) {
    __shared__ float bv[256];
    __shared__ int bi[256];
    __shared__ float red[4];
    const float* row = logits + (long long)blockIdx.x * N;
    float best = -INFINITY;
    int arg = 0x7FFFFFFF;
    for (int j = threadIdx.x; j < N; j += 256) {      // ascending j: the first maximum of the thread's columns
        const float v = row[j];
        if (v > best || arg == 0x7FFFFFFF) {
            best = v;
            arg = j;
        }
    }
    bv[threadIdx.x] = best;
    bi[threadIdx.x] = arg;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            const float v = bv[threadIdx.x + o];
            const int a = bi[threadIdx.x + o];
            if (a != 0x7FFFFFFF && (bi[threadIdx.x] == 0x7FFFFFFF || v > bv[threadIdx.x] || (v == bv[threadIdx.x] && a < bi[threadIdx.x]))) {
                bv[threadIdx.x] = v;
                bi[threadIdx.x] = a;
            }
        }
        __syncthreads();
    }
    const float mx = bv[0];
    const int am = bi[0];
    float s = 0.f;
    for (int j = threadIdx.x; j < N; j += 256) s += expf(row[j] - mx);
    s = block_sum_256(s, red);
    if (threadIdx.x == 0) {
        const int64_t l = label[blockIdx.x];
        const float e = mx + logf(s);
        lse[blockIdx.x] = e;
        loss[blockIdx.x] = (l >= 0 && l < N) ? e - row[l] : NAN;
        correct[blockIdx.x] = (l == am) ? 1.0f : 0.0f;
    }
}
__global__ __launch_bounds__(256) void softmax_ce_bwd_kernel(const float* __restrict__ dloss, const float* __restrict__ logits,
                                                             const int64_t* __restrict__ label, const float* __restrict__ lse,
                                                             float* __restrict__ dlogits, long long n, int N) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const long long b = i / N;
        const float p = expf(logits[i] - lse[b]);
        dlogits[i] = (p - (label[b] == i - b * N ? 1.0f : 0.0f)) * dloss[b];
    }
}

// ---------------------------------------------------------------- entry points
static int ir_check_rows(const char* what, int64_t M, int C) {
    GIM_CHECK_ARG(M > 0 && M < (1ll << 40) && C > 0 && C % 4 == 0 && C <= (1 << 18), what);
    return GIM_OK;
}

extern "C" int gim_bn_apply_fwd(const float* z, const float* gamma, const float* beta, const float* mean, const float* invstd,
                                const float* slope, float* y, int64_t M, int C, void* stream) {
    GIM_CHECK_ARG(z && gamma && beta && mean && invstd && y, "bn_apply_fwd: null pointer");
    if (ir_check_rows("bn_apply_fwd: bad dims (M > 0 rows, C % 4 == 0)", M, C)) return GIM_E_BADARG;
    GIM_CHECK_ARG(aligned16(z) && aligned16(gamma) && aligned16(beta) && aligned16(mean) && aligned16(invstd) && aligned16(slope) &&
                      aligned16(y), "bn_apply_fwd: pointers must be 16-byte aligned");
    const long long n4 = (long long)M * (C / 4);
    if (slope)
        hipLaunchKernelGGL(bn_apply_fwd_kernel<true>, dim3(blocks256(n4)), dim3(256), 0, (hipStream_t)stream, z, gamma, beta, mean, invstd,
                           slope, y, n4, C / 4);
    else
        hipLaunchKernelGGL(bn_apply_fwd_kernel<false>, dim3(blocks256(n4)), dim3(256), 0, (hipStream_t)stream, z, gamma, beta, mean, invstd,
                           slope, y, n4, C / 4);
    return gim_check_launch("gim_bn_apply_fwd");
}

extern "C" int gim_bn_bwd_reduce(const float* dy, const float* z, const float* gamma, const float* beta, const float* mean,
                                 const float* invstd, const float* slope, float* partials, float* dgamma, float* dbeta, float* dslope,
                                 float* acc_dgamma, float* acc_dbeta, float* acc_dslope, int64_t M, int C, void* stream) {
    GIM_CHECK_ARG(dy && z && gamma && beta && mean && invstd && partials && dgamma && dbeta, "bn_bwd_reduce: null pointer");
    GIM_CHECK_ARG(!slope == !dslope && (slope || !acc_dslope), "bn_bwd_reduce: slope and dslope are given together or not at all");
    if (ir_check_rows("bn_bwd_reduce: bad dims (M > 0 rows, C % 4 == 0)", M, C)) return GIM_E_BADARG;
    GIM_CHECK_ARG(aligned16(dy) && aligned16(z) && aligned16(gamma) && aligned16(beta) && aligned16(mean) && aligned16(invstd) &&
                      aligned16(slope) && aligned16(partials), "bn_bwd_reduce: pointers must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const long long rps = slab_rows(M);
    const int ns = slab_count(M);
    const dim3 grid((C + RS_CB - 1) / RS_CB, ns);
    if (slope)
        hipLaunchKernelGGL(bn_bwd_slab_kernel<true>, grid, dim3(256), 0, st, dy, z, gamma, beta, mean, invstd, slope, partials, (long long)M, C,
                           rps, ns);
    else
        hipLaunchKernelGGL(bn_bwd_slab_kernel<false>, grid, dim3(256), 0, st, dy, z, gamma, beta, mean, invstd, slope, partials, (long long)M,
                           C, rps, ns);
    rowsum_finalize(partials, ns, C, slope ? 3 : 2, dbeta, dgamma, dslope, acc_dbeta, acc_dgamma, acc_dslope, st);
    return gim_check_launch("gim_bn_bwd_reduce");
}

static int bn_bwd_dx(const char* name, const float* dy, const float* z, const float* gamma, const float* beta, const float* mean,
                     const float* invstd, const float* slope, const float* dgamma, const float* dbeta, float* dz, int64_t M, int C,
                     int64_t M_total, void* stream) {
    GIM_CHECK_ARG(dy && z && gamma && beta && mean && invstd && dgamma && dbeta && dz, "bn_bwd_dx: null pointer");
    if (ir_check_rows("bn_bwd_dx: bad dims (M > 0 rows, C % 4 == 0)", M, C)) return GIM_E_BADARG;
    GIM_CHECK_ARG(aligned16(dy) && aligned16(z) && aligned16(gamma) && aligned16(beta) && aligned16(mean) && aligned16(invstd) &&
                      aligned16(slope) && aligned16(dgamma) && aligned16(dbeta) && aligned16(dz),
                  "bn_bwd_dx: pointers must be 16-byte aligned");
    const long long n4 = (long long)M * (C / 4);
    const float inv_m = 1.0f / (float)M_total;
    if (slope)
        hipLaunchKernelGGL(bn_bwd_dx_kernel<true>, dim3(blocks256(n4)), dim3(256), 0, (hipStream_t)stream, dy, z, gamma, beta, mean, invstd,
                           slope, dgamma, dbeta, dz, n4, C / 4, inv_m);
    else
        hipLaunchKernelGGL(bn_bwd_dx_kernel<false>, dim3(blocks256(n4)), dim3(256), 0, (hipStream_t)stream, dy, z, gamma, beta, mean, invstd,
                           slope, dgamma, dbeta, dz, n4, C / 4, inv_m);
    return gim_check_launch(name);
}

extern "C" int gim_bn_bwd_dx(const float* dy, const float* z, const float* gamma, const float* beta, const float* mean, const float* invstd,
                             const float* slope, const float* dgamma, const float* dbeta, float* dz, int64_t M, int C, void* stream) {
    return bn_bwd_dx("gim_bn_bwd_dx", dy, z, gamma, beta, mean, invstd, slope, dgamma, dbeta, dz, M, C, M, stream);
}

extern "C" int gim_bn_bwd_dx_total(const float* dy, const float* z, const float* gamma, const float* beta, const float* mean,
                                   const float* invstd, const float* slope, const float* dgamma, const float* dbeta, float* dz, int64_t M,
                                   int64_t M_total, int C, void* stream) {
    GIM_CHECK_ARG(M_total >= M && M_total < (1ll << 40), "bn_bwd_dx_total: M_total must be at least the M rows of z");
    return bn_bwd_dx("gim_bn_bwd_dx_total", dy, z, gamma, beta, mean, invstd, slope, dgamma, dbeta, dz, M, C, M_total, stream);
}

extern "C" int gim_prelu_fwd(const float* x, const float* slope, float* y, int64_t M, int C, void* stream) {
    GIM_CHECK_ARG(x && y, "prelu_fwd: null pointer");
    if (ir_check_rows("prelu_fwd: bad dims (M > 0 rows, C % 4 == 0)", M, C)) return GIM_E_BADARG;
    GIM_CHECK_ARG(aligned16(x) && aligned16(slope) && aligned16(y), "prelu_fwd: pointers must be 16-byte aligned");
    const long long n4 = (long long)M * (C / 4);
    if (slope)
        hipLaunchKernelGGL(prelu_fwd_kernel<true>, dim3(blocks256(n4)), dim3(256), 0, (hipStream_t)stream, x, slope, y, n4, C / 4);
    else
        hipLaunchKernelGGL(prelu_fwd_kernel<false>, dim3(blocks256(n4)), dim3(256), 0, (hipStream_t)stream, x, slope, y, n4, C / 4);
    return gim_check_launch("gim_prelu_fwd");
}

extern "C" int gim_prelu_bwd(const float* dy, const float* x, const float* slope, float* dx, float* partials, float* dslope,
                             float* acc_dslope, int64_t M, int C, void* stream) {
    GIM_CHECK_ARG(dy && x && dx, "prelu_bwd: null pointer");
    GIM_CHECK_ARG(slope ? (partials && dslope) : (!dslope && !acc_dslope), "prelu_bwd: slope, partials and dslope are given together or not at all");
    if (ir_check_rows("prelu_bwd: bad dims (M > 0 rows, C % 4 == 0)", M, C)) return GIM_E_BADARG;
    GIM_CHECK_ARG(aligned16(dy) && aligned16(x) && aligned16(slope) && aligned16(dx) && aligned16(partials),
                  "prelu_bwd: pointers must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const long long rps = slab_rows(M);
    const int ns = slab_count(M);
    const dim3 grid((C + RS_CB - 1) / RS_CB, ns);
    if (slope) {
        hipLaunchKernelGGL(prelu_bwd_slab_kernel<true>, grid, dim3(256), 0, st, dy, x, slope, dx, partials, (long long)M, C, rps, ns);
        rowsum_finalize(partials, ns, C, 1, dslope, nullptr, nullptr, acc_dslope, nullptr, nullptr, st);
    } else {
        hipLaunchKernelGGL(prelu_bwd_slab_kernel<false>, grid, dim3(256), 0, st, dy, x, slope, dx, partials, (long long)M, C, rps, ns);
    }
    return gim_check_launch("gim_prelu_bwd");
}

extern "C" int gim_se_tail_bwd(const float* dout, const float* res, const float* gate, float* dres, float* dgate, int N, int Ho, int Wo,
                               int C, void* stream) {
    GIM_CHECK_ARG(dout && res && gate && dres && dgate, "se_tail_bwd: null pointer");
    GIM_CHECK_ARG(N > 0 && N <= 65535 && Ho > 0 && Wo > 0 && (long long)Ho * Wo < (1ll << 31) && C > 0 && C % 4 == 0 && C <= (1 << 18),
                  "se_tail_bwd: bad dims (N <= 65535, C % 4 == 0)");
    GIM_CHECK_ARG(aligned16(dout) && aligned16(res) && aligned16(gate) && aligned16(dres) && aligned16(dgate),
                  "se_tail_bwd: pointers must be 16-byte aligned");
    hipLaunchKernelGGL(se_tail_bwd_kernel, dim3((C + RS_CB - 1) / RS_CB, N), dim3(256), 0, (hipStream_t)stream, dout, res, gate, dres, dgate,
                       Ho * Wo, C);
    return gim_check_launch("gim_se_tail_bwd");
}

extern "C" int gim_subsample2_fwd(const float* x, float* y, int N, int H, int W, int C, void* stream) {
    GIM_CHECK_ARG(x && y && N > 0 && H >= 2 && W >= 2 && !(H & 1) && !(W & 1) && C > 0 && C % 4 == 0,
                  "subsample2_fwd: bad args (H, W even: the INPUT size; C % 4 == 0)");
    GIM_CHECK_ARG(aligned16(x) && aligned16(y), "subsample2_fwd: pointers must be 16-byte aligned");
    const long long n4 = (long long)N * (H / 2) * (W / 2) * (C / 4);
    hipLaunchKernelGGL(subsample2_fwd_kernel, dim3(blocks256(n4)), dim3(256), 0, (hipStream_t)stream, x, y, n4, H / 2, W / 2, C / 4);
    return gim_check_launch("gim_subsample2_fwd");
}

extern "C" int gim_subsample2_bwd(const float* dy, float* dx, int N, int H, int W, int C, void* stream) {
    GIM_CHECK_ARG(dy && dx && N > 0 && H >= 2 && W >= 2 && !(H & 1) && !(W & 1) && C > 0 && C % 4 == 0,
                  "subsample2_bwd: bad args (H, W even: the size of dx; C % 4 == 0)");
    GIM_CHECK_ARG(aligned16(dy) && aligned16(dx), "subsample2_bwd: pointers must be 16-byte aligned");
    const long long n4 = (long long)N * H * W * (C / 4);
    hipLaunchKernelGGL(subsample2_bwd_kernel, dim3(blocks256(n4)), dim3(256), 0, (hipStream_t)stream, dy, dx, n4, H, W, C / 4);
    return gim_check_launch("gim_subsample2_bwd");
}

extern "C" int gim_dropout(const float* x, float* y, int64_t n, float p, uint64_t seed, uint64_t offset, void* stream) {
    GIM_CHECK_ARG(x && y && n > 0 && n % 4 == 0, "dropout: bad args (n % 4 == 0)");
    GIM_CHECK_ARG(p >= 0.f && p < 1.f, "dropout: p must be in [0, 1)");
    GIM_CHECK_ARG(aligned16(x) && aligned16(y), "dropout: pointers must be 16-byte aligned");
    // p == 0: every hash value is >= 0 and the scale is exactly 1 - the copy is bit-exact
    hipLaunchKernelGGL(dropout_kernel, dim3(blocks256(n / 4)), dim3(256), 0, (hipStream_t)stream, x, y, (long long)(n / 4), p,
                       1.0f / (1.0f - p), seed, offset);
    return gim_check_launch("gim_dropout");
}

extern "C" int gim_l2norm_rows_bwd(const float* dy, const float* x, float* dx, int B, int D, void* stream) {
    GIM_CHECK_ARG(dy && x && dx && B > 0 && D > 0 && D % 4 == 0, "l2norm_rows_bwd: bad args (D % 4 == 0)");
    GIM_CHECK_ARG(aligned16(dy) && aligned16(x) && aligned16(dx), "l2norm_rows_bwd: pointers must be 16-byte aligned");
    hipLaunchKernelGGL(l2norm_rows_bwd_kernel, dim3((B + 3) / 4), dim3(256), 0, (hipStream_t)stream, dy, x, dx, B, D / 4);
    return gim_check_launch("gim_l2norm_rows_bwd");
}

extern "C" int gim_col_l2norm_fwd(const float* k, float* out, int E, int N, void* stream) {
    GIM_CHECK_ARG(k && out && E > 0 && N > 0, "col_l2norm_fwd: bad args");
    hipLaunchKernelGGL(col_l2norm_fwd_kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, k, out, E, N);
    return gim_check_launch("gim_col_l2norm_fwd");
}

extern "C" int gim_col_l2norm_bwd(const float* dn, const float* k, float* dk, int E, int N, void* stream) {
    GIM_CHECK_ARG(dn && k && dk && E > 0 && N > 0, "col_l2norm_bwd: bad args");
    hipLaunchKernelGGL(col_l2norm_bwd_kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, dn, k, dk, E, N);
    return gim_check_launch("gim_col_l2norm_bwd");
}

extern "C" int gim_arcface_margin_fwd(const float* cosv, const int64_t* label, float* out, int B, int N, float s, float cos_m, float sin_m,
                                      float mm, float threshold, void* stream) {
    GIM_CHECK_ARG(cosv && label && out && B > 0 && N > 0 && s > 0.f, "arcface_margin_fwd: bad args");
    const IrMargin m = {s, cos_m, sin_m, mm, threshold};
    const long long n = (long long)B * N;
    hipLaunchKernelGGL(arc_margin_fwd_kernel, dim3(blocks256(n)), dim3(256), 0, (hipStream_t)stream, cosv, label, out, n, N, m);
    return gim_check_launch("gim_arcface_margin_fwd");
}

extern "C" int gim_arcface_margin_bwd(const float* dout, const float* cosv, const int64_t* label, float* dcos, int B, int N, float s,
                                      float cos_m, float sin_m, float mm, float threshold, void* stream) {
    GIM_CHECK_ARG(dout && cosv && label && dcos && B > 0 && N > 0 && s > 0.f, "arcface_margin_bwd: bad args");
    const IrMargin m = {s, cos_m, sin_m, mm, threshold};
    const long long n = (long long)B * N;
    hipLaunchKernelGGL(arc_margin_bwd_kernel, dim3(blocks256(n)), dim3(256), 0, (hipStream_t)stream, dout, cosv, label, dcos, n, N, m);
    return gim_check_launch("gim_arcface_margin_bwd");
}

extern "C" int gim_softmax_ce_fwd(const float* logits, const int64_t* label, float* loss, float* correct, float* lse, int B, int N,
                                  void* stream) {
    GIM_CHECK_ARG(logits && label && loss && correct && lse && B > 0 && N > 0, "softmax_ce_fwd: bad args");
    hipLaunchKernelGGL(softmax_ce_fwd_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, logits, label, loss, correct, lse, N);
    return gim_check_launch("gim_softmax_ce_fwd");
}

extern "C" int gim_softmax_ce_bwd(const float* dloss, const float* logits, const int64_t* label, const float* lse, float* dlogits, int B,
                                  int N, void* stream) {
    GIM_CHECK_ARG(dloss && logits && label && lse && dlogits && B > 0 && N > 0, "softmax_ce_bwd: bad args");
    const long long n = (long long)B * N;
    hipLaunchKernelGGL(softmax_ce_bwd_kernel, dim3(blocks256(n)), dim3(256), 0, (hipStream_t)stream, dloss, logits, label, lse, dlogits, n, N);
    return gim_check_launch("gim_softmax_ce_bwd");
}
