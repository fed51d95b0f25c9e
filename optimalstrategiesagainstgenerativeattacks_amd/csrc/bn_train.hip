// BatchNorm2d with BATCH statistics fused with the ReLU and the 2x2 max pool behind it, forward and backward, plus the backward of
// |a - b|: what training the siamese baseline (baseline_training.py; siamese/models.py:50-56,106-109) needs beyond the convolutions.
// NHWC fp32, C % 4 == 0, every base pointer 16-byte aligned (checked by the entry points): one thread moves 16 bytes (4 channels)
// per access, lanes run along the channel axis.  All of it is bandwidth-bound; the passes over the full-resolution map z are
// one for the statistics, one for the forward, two for the backward (the per-channel sums, then dz).
//
// No float atomics and no allocation: a sum over all rows of a map goes through the caller's `partials` buffer - stage 1 gives each
// workgroup a slab of rows and writes one partial per channel, stage 2 (one small launch) combines the partials of a channel in a
// fixed order.  Two runs are bit-identical.
//
// Variance: never E[x^2] - E[x]^2 over the map.  A slab sums (x - K) and (x - K)^2 about a per-channel shift K taken from the DATA
// (the slab's first row), which gives the slab's (count, mean, M2) with a cancellation of the order (mean_slab - K)^2 / var_slab = O(1)
// whatever the offset of the map; stage 2 combines the slabs' triples with Chan's formula.
//
// The arg-max of a pooling window is RECOMPUTED in the backward from the four z values (the backward reads z anyway for xhat), not
// stored by the forward.  The affine is applied to each of the four values before the maximum (gamma may be negative); ties go to the
// first maximum in row-major window order, as torch.nn.MaxPool2d.
#include "common.h"

#define BN_MAX_SLABS 1024
#define BN_MIN_SLAB_ROWS 64
#define BN_MAX_BLOCKS 4096
constexpr int BN_CB = 64;             // channels per workgroup of a slab kernel
constexpr int BN_CL = BN_CB / 4;      // lanes along channels (16 bytes each)
constexpr int BN_HG = 256 / BN_CL;    // thread groups along rows
constexpr int BN_FC = 4;              // channels per workgroup of a finalize kernel ...
constexpr int BN_FG = 256 / BN_FC;    // ... x 64 groups of at most BN_MAX_SLABS / 64 consecutive slabs

static inline bool bn_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }
static inline int bn_blocks(long long n) {
    long long b = (n + 255) / 256;
    return (int)(b > BN_MAX_BLOCKS ? BN_MAX_BLOCKS : (b < 1 ? 1 : b));
}
// rows per slab; the slab count is ceil(rows / bn_slab_rows(rows)): no slab is empty
static inline long long bn_slab_rows(long long rows) {
    long long ns = (rows + BN_MIN_SLAB_ROWS - 1) / BN_MIN_SLAB_ROWS;
    if (ns > BN_MAX_SLABS) ns = BN_MAX_SLABS;
    if (ns < 1) ns = 1;
    return (rows + ns - 1) / ns;
}
static inline int bn_slab_count(long long rows) {
    const long long rps = bn_slab_rows(rows);
    return (int)((rows + rps - 1) / rps);
}

__device__ __forceinline__ f32x4 bn_ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void bn_st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

// sum of two quads per thread over the BN_HG thread groups, in group order; valid in the threads of group 0
__device__ __forceinline__ void bn_group_sum2(f32x4& a, f32x4& b, float (*red)[BN_HG * BN_CB], int cl, int hg) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        red[0][hg * BN_CB + cl * 4 + e] = a[e];
        red[1][hg * BN_CB + cl * 4 + e] = b[e];
    }
    __syncthreads();
    if (hg == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float sa = 0.f, sb = 0.f;
            for (int g = 0; g < BN_HG; ++g) {
                sa += red[0][g * BN_CB + cl * 4 + e];
                sb += red[1][g * BN_CB + cl * 4 + e];
            }
            a[e] = sa;
            b[e] = sb;
        }
    }
}

// ---------------------------------------------------------------- statistics, stage 1: (mean, M2) of one slab of rows per channel
__global__ __launch_bounds__(256) void bn_stats_slab_kernel(const float* __restrict__ z, float* __restrict__ partials, long long M, int C,
                                                            long long rps) {
    __shared__ float red[2][BN_HG * BN_CB];
    const int cl = threadIdx.x % BN_CL, hg = threadIdx.x / BN_CL;
    const int c = blockIdx.x * BN_CB + cl * 4;
    const long long r0 = (long long)blockIdx.y * rps;
    const long long r1 = (r0 + rps < M) ? r0 + rps : M;
    const bool ok = c < C;
    f32x4 K = {0.f, 0.f, 0.f, 0.f}, s1 = K, s2 = K;
    if (ok) {
        K = bn_ld4(z + r0 * C + c);
#pragma unroll 8
        for (long long r = r0 + hg; r < r1; r += BN_HG) {     // (8 independent 16-byte loads in flight per lane)
            const f32x4 d = bn_ld4(z + r * C + c) - K;
            s1 += d;
            s2 += d * d;
        }
    }
    bn_group_sum2(s1, s2, red, cl, hg);
    if (ok && hg == 0) {
        const float inv_n = 1.0f / (float)(r1 - r0);
        float* out = partials + ((long long)blockIdx.y * C + c) * 2;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float m = s1[e] * inv_n;
            out[2 * e] = K[e] + m;
            out[2 * e + 1] = fmaxf(s2[e] - s1[e] * m, 0.f);
        }
    }
}

// ---------------------------------------------------------------- stage 2 of both sums: 4 channels x 64 groups of consecutive slabs
// STATS: partials hold (mean, M2) of slabs of `rps` rows (the last one shorter), combined with Chan's formula; otherwise plain sums.
// Always in the same order: a thread combines its group's <= 16 slabs in slab order (their loads are all in flight at once: the
// partials were just written by other CUs, a dependent chain of 64 such loads took longer than stage 1 at the smaller maps), then
// every eighth thread its 8 neighbouring groups, then one thread those 8 results.  STATS: out0 = mean, out1 = invstd, and the running
// statistics move; otherwise out0 / out1 the two totals, also ADDED to acc0 / acc1 where given (a parameter's .grad).
struct BnAcc {
    float n, a, b;     // STATS: count, mean, M2; otherwise a, b the two sums (n unused)
};
template <bool STATS>
__device__ __forceinline__ void bn_combine(BnAcc& t, float nb, float pa, float pb) {
    if (STATS) {
        if (nb > 0.f) {
            const float nn = t.n + nb, d = pa - t.a, w = nb / nn;
            t.a += d * w;
            t.b += pb + d * d * (t.n * w);
            t.n = nn;
        }
    } else {
        t.a += pa;
        t.b += pb;
    }
}
template <bool STATS>
__global__ __launch_bounds__(256) void bn_finalize_kernel(const float* __restrict__ partials, int n_slabs, long long rps, long long M, int C,
                                                          float* __restrict__ out0, float* __restrict__ out1, float* __restrict__ acc0,
                                                          float* __restrict__ acc1, long long* __restrict__ nbt, float momentum, float eps) {
    __shared__ float red[3][BN_FG * BN_FC];
    const int ci = threadIdx.x % BN_FC, g = threadIdx.x / BN_FC;
    const int c = blockIdx.x * BN_FC + ci;
    const int per = (n_slabs + BN_FG - 1) / BN_FG;      // <= 16
    const int s0 = g * per;
    BnAcc t = {0.f, 0.f, 0.f};
    if (c < C) {
        float pa[BN_MAX_SLABS / BN_FG], pb[BN_MAX_SLABS / BN_FG];
#pragma unroll
        for (int k = 0; k < BN_MAX_SLABS / BN_FG; ++k) {
            const bool in = k < per && s0 + k < n_slabs;
            const float* p = partials + ((long long)(in ? s0 + k : 0) * C + c) * 2;
            pa[k] = p[0];
            pb[k] = p[1];
        }
#pragma unroll
        for (int k = 0; k < BN_MAX_SLABS / BN_FG; ++k) {
            const long long lo = (long long)(s0 + k) * rps;
            const bool in = k < per && s0 + k < n_slabs;
            const float nb = in ? (float)(((lo + rps < M) ? lo + rps : M) - lo) : 0.f;
            bn_combine<STATS>(t, nb, in ? pa[k] : 0.f, in ? pb[k] : 0.f);
        }
    }
    red[0][g * BN_FC + ci] = t.n;
    red[1][g * BN_FC + ci] = t.a;
    red[2][g * BN_FC + ci] = t.b;
    __syncthreads();
    if ((g & 7) == 0)
        for (int k = 1; k < 8; ++k) bn_combine<STATS>(t, red[0][(g + k) * BN_FC + ci], red[1][(g + k) * BN_FC + ci], red[2][(g + k) * BN_FC + ci]);
    __syncthreads();
    if ((g & 7) == 0) {
        red[0][g * BN_FC + ci] = t.n;
        red[1][g * BN_FC + ci] = t.a;
        red[2][g * BN_FC + ci] = t.b;
    }
    __syncthreads();
    if (g != 0 || c >= C) return;
    for (int k = 8; k < BN_FG; k += 8) bn_combine<STATS>(t, red[0][k * BN_FC + ci], red[1][k * BN_FC + ci], red[2][k * BN_FC + ci]);
    const float a = t.a, b = t.b;
    if (STATS) {
        const float var = b / (float)M;
        out0[c] = a;
        out1[c] = 1.0f / sqrtf(var + eps);
        if (acc0) {   // running_mean, running_var (the unbiased estimate)
            acc0[c] = (1.0f - momentum) * acc0[c] + momentum * a;
            acc1[c] = (1.0f - momentum) * acc1[c] + momentum * (b / (float)(M - 1));
        }
        if (nbt && c == 0) *nbt += 1;
    } else {
        out0[c] = a;
        out1[c] = b;
        if (acc0) acc0[c] += a;
        if (acc1) acc1[c] += b;
    }
}

// ---------------------------------------------------------------- one pooling window of one channel quad
struct BnChan {
    f32x4 mean, invstd, s, beta;   // s = gamma * invstd
};
__device__ __forceinline__ BnChan bn_chan(const float* gamma, const float* beta, const float* mean, const float* invstd, int c) {
    BnChan p;
    p.mean = bn_ld4(mean + c);
    p.invstd = bn_ld4(invstd + c);
    p.s = bn_ld4(gamma + c) * p.invstd;
    p.beta = bn_ld4(beta + c);
    return p;
}
// the four values of the window at zp (rows `row` floats apart, columns C floats), normalised; best / arg: the maximum of the affine
// values and its position 0..3 in row-major order (the first one on a tie)
__device__ __forceinline__ void bn_window(const float* zp, long long row, int C, const BnChan& p, f32x4 (&xh)[4], f32x4& best, int (&arg)[4]) {
    const f32x4 v[4] = {bn_ld4(zp), bn_ld4(zp + C), bn_ld4(zp + row), bn_ld4(zp + row + C)};
#pragma unroll
    for (int k = 0; k < 4; ++k) xh[k] = v[k] - p.mean;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        best[q] = fmaf(xh[0][q], p.s[q], p.beta[q]);
        arg[q] = 0;
#pragma unroll
        for (int k = 1; k < 4; ++k) {
            const float y = fmaf(xh[k][q], p.s[q], p.beta[q]);
            if (y > best[q]) {
                best[q] = y;
                arg[q] = k;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) xh[k] *= p.invstd;
}
// pooled row r (= (n * Ho + i) * Wo + j) -> offset of its window's first pixel in z, in floats (without the channel)
__device__ __forceinline__ long long bn_window_base(long long r, int Ho, int Wo, int W, int C) {
    const int j = (int)(r % Wo);
    const long long t = r / Wo;
    const int i = (int)(t % Ho);
    const long long n = t / Ho;
    return (((n * Ho + i) * 2) * W + 2 * j) * C;
}

// ---------------------------------------------------------------- forward: p = maxpool2(relu(bn(z)))
__global__ __launch_bounds__(256) void bn_relu_maxpool2_fwd_kernel(const float* __restrict__ z, const float* __restrict__ gamma,
                                                                   const float* __restrict__ beta, const float* __restrict__ mean,
                                                                   const float* __restrict__ invstd, float* __restrict__ out, long long Mp,
                                                                   int Ho, int Wo, int C) {
    const int C4 = C >> 2, W = Wo * 2;
    const long long n_out = Mp * C4, row = (long long)W * C;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_out; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % C4) * 4;
        const BnChan p = bn_chan(gamma, beta, mean, invstd, c);
        f32x4 xh[4], best;
        int arg[4];
        bn_window(z + bn_window_base(i / C4, Ho, Wo, W, C) + c, row, C, p, xh, best, arg);
#pragma unroll
        for (int q = 0; q < 4; ++q) best[q] = fmaxf(best[q], 0.f);
        bn_st4(out + i * 4, best);
    }
}

// ---------------------------------------------------------------- backward, stage 1 of the sums: per slab of POOLED rows
// (sum dyhat, sum dyhat * xhat), dyhat = dp at the window's arg-max where that maximum is > 0
__global__ __launch_bounds__(256) void bn_pool_bwd_slab_kernel(const float* __restrict__ dp, const float* __restrict__ z,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta,
                                                               const float* __restrict__ mean, const float* __restrict__ invstd,
                                                               float* __restrict__ partials, long long Mp, int Ho, int Wo, int C, long long rps) {
    __shared__ float red[2][BN_HG * BN_CB];
    const int cl = threadIdx.x % BN_CL, hg = threadIdx.x / BN_CL;
    const int c = blockIdx.x * BN_CB + cl * 4;
    const int W = Wo * 2;
    const long long row = (long long)W * C;
    const long long r0 = (long long)blockIdx.y * rps;
    const long long r1 = (r0 + rps < Mp) ? r0 + rps : Mp;
    const bool ok = c < C;
    f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = s1;
    if (ok) {
        const BnChan p = bn_chan(gamma, beta, mean, invstd, c);
#pragma unroll 2
        for (long long r = r0 + hg; r < r1; r += BN_HG) {
            f32x4 xh[4], best;
            int arg[4];
            const f32x4 g = bn_ld4(dp + r * C + c);
            bn_window(z + bn_window_base(r, Ho, Wo, W, C) + c, row, C, p, xh, best, arg);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float xa = xh[0][q];
#pragma unroll
                for (int k = 1; k < 4; ++k) xa = (arg[q] == k) ? xh[k][q] : xa;
                const float d = best[q] > 0.f ? g[q] : 0.f;
                s1[q] += d;
                s2[q] += d * xa;
            }
        }
    }
    bn_group_sum2(s1, s2, red, cl, hg);
    if (ok && hg == 0) {
        float* out = partials + ((long long)blockIdx.y * C + c) * 2;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            out[2 * e] = s1[e];
            out[2 * e + 1] = s2[e];
        }
    }
}

// ---------------------------------------------------------------- backward: dz = gamma * invstd * (dyhat - dbeta / M - xhat * dgamma / M)
__global__ __launch_bounds__(256) void bn_pool_bwd_dx_kernel(const float* __restrict__ dp, const float* __restrict__ z,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             const float* __restrict__ mean, const float* __restrict__ invstd,
                                                             const float* __restrict__ dgamma, const float* __restrict__ dbeta,
                                                             float* __restrict__ dz, long long Mp, int Ho, int Wo, int C) {
    const int C4 = C >> 2, W = Wo * 2;
    const long long n_out = Mp * C4, row = (long long)W * C;
    const float inv_m = 1.0f / (float)(Mp * 4);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_out; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % C4) * 4;
        const BnChan p = bn_chan(gamma, beta, mean, invstd, c);
        const f32x4 mb = bn_ld4(dbeta + c) * inv_m, mg = bn_ld4(dgamma + c) * inv_m;
        const f32x4 g = bn_ld4(dp + i * 4);
        f32x4 xh[4], best;
        int arg[4];
        const long long base = bn_window_base(i / C4, Ho, Wo, W, C) + c;
        bn_window(z + base, row, C, p, xh, best, arg);
        f32x4 o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float d = (arg[q] == k && best[q] > 0.f) ? g[q] : 0.f;
                o[k][q] = p.s[q] * (d - mb[q] - xh[k][q] * mg[q]);
            }
        bn_st4(dz + base, o[0]);
        bn_st4(dz + base + C, o[1]);
        bn_st4(dz + base + row, o[2]);
        bn_st4(dz + base + row + C, o[3]);
    }
}

// ---------------------------------------------------------------- da = sign(a - b) * d, db = -da
__global__ __launch_bounds__(256) void absdiff_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ d,
                                                          float* __restrict__ da, float* __restrict__ db, long long n4) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const f32x4 va = bn_ld4(a + i * 4), vb = bn_ld4(b + i * 4), vd = bn_ld4(d + i * 4);
        f32x4 ga, gb;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float t = va[q] - vb[q];
            ga[q] = t > 0.f ? vd[q] : (t < 0.f ? -vd[q] : 0.f);
            gb[q] = -ga[q];
        }
        bn_st4(da + i * 4, ga);
        bn_st4(db + i * 4, gb);
    }
}

// ---------------------------------------------------------------- share of logits on the right side of 0: rows < n_pos are positives
__global__ __launch_bounds__(256) void logit_accuracy_kernel(const float* __restrict__ logits, int n_pos, int n, float* __restrict__ out) {
    __shared__ float red[4];
    float cnt = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) cnt += ((logits[i] >= 0.f) == (i < n_pos)) ? 1.f : 0.f;
    cnt = block_sum_256(cnt, red);     // integers below 2^24: exact in any order
    if (threadIdx.x == 0) out[0] = cnt / (float)n;
}

// ---------------------------------------------------------------- entry points
extern "C" int gim_bn_slabs(int64_t rows) {
    GIM_CHECK_ARG(rows > 0, "bn_slabs: rows must be positive");
    return bn_slab_count(rows);
}

extern "C" int gim_bn_partials_floats(int64_t rows, int C) {
    GIM_CHECK_ARG(rows > 0 && C > 0 && C <= (1 << 18), "bn_partials_floats: bad args");
    return bn_slab_count(rows) * C * 2;
}

static int bn_check_map(const char* what, int N, int H, int W, int C) {
    GIM_CHECK_ARG(N > 0 && H >= 2 && W >= 2 && !(H & 1) && !(W & 1) && C > 0 && C % 4 == 0 && C <= (1 << 18), what);
    return GIM_OK;
}

extern "C" int gim_bn_stats(const float* z, float* partials, float* mean, float* invstd, float* running_mean, float* running_var,
                            int64_t* num_batches_tracked, int64_t M, int C, float momentum, float eps, void* stream) {
    GIM_CHECK_ARG(z && partials && mean && invstd, "bn_stats: null pointer");
    GIM_CHECK_ARG(M >= 2 && C > 0 && C % 4 == 0 && C <= (1 << 18), "bn_stats: bad dims (M >= 2 rows, C % 4 == 0)");
    GIM_CHECK_ARG(!running_mean == !running_var, "bn_stats: running_mean and running_var are given together or not at all");
    GIM_CHECK_ARG(bn_aligned(z), "bn_stats: z must be 16-byte aligned");
    GIM_CHECK_ARG(momentum >= 0.f && momentum <= 1.f && eps >= 0.f, "bn_stats: momentum in [0, 1], eps >= 0");
    hipStream_t st = (hipStream_t)stream;
    const long long rps = bn_slab_rows(M);
    const int ns = bn_slab_count(M);
    hipLaunchKernelGGL(bn_stats_slab_kernel, dim3((C + BN_CB - 1) / BN_CB, ns), dim3(256), 0, st, z, partials, (long long)M, C, rps);
    hipLaunchKernelGGL((bn_finalize_kernel<true>), dim3((C + BN_FC - 1) / BN_FC), dim3(256), 0, st, partials, ns, rps, (long long)M, C, mean,
                       invstd, running_mean, running_var, (long long*)num_batches_tracked, momentum, eps);
    return gim_check_launch("gim_bn_stats");
}

extern "C" int gim_bn_relu_maxpool2_fwd(const float* z, const float* gamma, const float* beta, const float* mean, const float* invstd,
                                        float* p, int N, int H, int W, int C, void* stream) {
    GIM_CHECK_ARG(z && gamma && beta && mean && invstd && p, "bn_relu_maxpool2_fwd: null pointer");
    if (bn_check_map("bn_relu_maxpool2_fwd: bad dims (H, W even, C % 4 == 0)", N, H, W, C)) return GIM_E_BADARG;
    GIM_CHECK_ARG(bn_aligned(z) && bn_aligned(gamma) && bn_aligned(beta) && bn_aligned(mean) && bn_aligned(invstd) && bn_aligned(p),
                  "bn_relu_maxpool2_fwd: pointers must be 16-byte aligned");
    const long long Mp = (long long)N * (H / 2) * (W / 2);
    hipLaunchKernelGGL(bn_relu_maxpool2_fwd_kernel, dim3(bn_blocks(Mp * (C / 4))), dim3(256), 0, (hipStream_t)stream, z, gamma, beta, mean,
                       invstd, p, Mp, H / 2, W / 2, C);
    return gim_check_launch("gim_bn_relu_maxpool2_fwd");
}

extern "C" int gim_bn_pool_bwd_reduce(const float* dp, const float* z, const float* gamma, const float* beta, const float* mean,
                                      const float* invstd, float* partials, float* dgamma, float* dbeta, float* acc_dgamma,
                                      float* acc_dbeta, int N, int H, int W, int C, void* stream) {
    GIM_CHECK_ARG(dp && z && gamma && beta && mean && invstd && partials && dgamma && dbeta, "bn_pool_bwd_reduce: null pointer");
    if (bn_check_map("bn_pool_bwd_reduce: bad dims (H, W even, C % 4 == 0)", N, H, W, C)) return GIM_E_BADARG;
    GIM_CHECK_ARG(bn_aligned(dp) && bn_aligned(z) && bn_aligned(gamma) && bn_aligned(beta) && bn_aligned(mean) && bn_aligned(invstd),
                  "bn_pool_bwd_reduce: pointers must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const long long Mp = (long long)N * (H / 2) * (W / 2);
    const long long rps = bn_slab_rows(Mp);
    const int ns = bn_slab_count(Mp);
    hipLaunchKernelGGL(bn_pool_bwd_slab_kernel, dim3((C + BN_CB - 1) / BN_CB, ns), dim3(256), 0, st, dp, z, gamma, beta, mean, invstd, partials,
                       Mp, H / 2, W / 2, C, rps);
    hipLaunchKernelGGL((bn_finalize_kernel<false>), dim3((C + BN_FC - 1) / BN_FC), dim3(256), 0, st, partials, ns, rps, Mp, C, dbeta, dgamma,
                       acc_dbeta, acc_dgamma, (long long*)nullptr, 0.f, 0.f);
    return gim_check_launch("gim_bn_pool_bwd_reduce");
}

extern "C" int gim_bn_pool_bwd_dx(const float* dp, const float* z, const float* gamma, const float* beta, const float* mean,
                                  const float* invstd, const float* dgamma, const float* dbeta, float* dz, int N, int H, int W, int C,
                                  void* stream) {
    GIM_CHECK_ARG(dp && z && gamma && beta && mean && invstd && dgamma && dbeta && dz, "bn_pool_bwd_dx: null pointer");
    if (bn_check_map("bn_pool_bwd_dx: bad dims (H, W even, C % 4 == 0)", N, H, W, C)) return GIM_E_BADARG;
    GIM_CHECK_ARG(bn_aligned(dp) && bn_aligned(z) && bn_aligned(gamma) && bn_aligned(beta) && bn_aligned(mean) && bn_aligned(invstd) &&
                      bn_aligned(dgamma) && bn_aligned(dbeta) && bn_aligned(dz),
                  "bn_pool_bwd_dx: pointers must be 16-byte aligned");
    const long long Mp = (long long)N * (H / 2) * (W / 2);
    hipLaunchKernelGGL(bn_pool_bwd_dx_kernel, dim3(bn_blocks(Mp * (C / 4))), dim3(256), 0, (hipStream_t)stream, dp, z, gamma, beta, mean, invstd,
                       dgamma, dbeta, dz, Mp, H / 2, W / 2, C);
    return gim_check_launch("gim_bn_pool_bwd_dx");
}

extern "C" int gim_absdiff_bwd(const float* a, const float* b, const float* d, float* da, float* db, int64_t n, void* stream) {
    GIM_CHECK_ARG(a && b && d && da && db && n > 0 && n % 4 == 0, "absdiff_bwd: bad args (n % 4 == 0)");
    GIM_CHECK_ARG(bn_aligned(a) && bn_aligned(b) && bn_aligned(d) && bn_aligned(da) && bn_aligned(db),
                  "absdiff_bwd: pointers must be 16-byte aligned");
    hipLaunchKernelGGL(absdiff_bwd_kernel, dim3(bn_blocks(n / 4)), dim3(256), 0, (hipStream_t)stream, a, b, d, da, db, (long long)(n / 4));
    return gim_check_launch("gim_absdiff_bwd");
}

extern "C" int gim_logit_accuracy(const float* logits, int n_pos, int n, float* out, void* stream) {
    GIM_CHECK_ARG(logits && out && n > 0 && n_pos >= 0 && n_pos <= n && n < (1 << 24), "logit_accuracy: bad args");
    hipLaunchKernelGGL(logit_accuracy_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, logits, n_pos, n, out);
    return gim_check_launch("gim_logit_accuracy");
}
