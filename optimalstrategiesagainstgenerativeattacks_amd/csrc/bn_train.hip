// BatchNorm2d with BATCH statistics fused with the ReLU and the 2x2 max pool behind it, forward and backward, plus the backward of
// |a - b|: what training the siamese baseline (baseline_training.py; siamese/models.py:50-56,106-109) needs beyond the convolutions.
// NHWC fp32, C % 4 == 0, every base pointer 16-byte aligned (checked by the entry points): one thread moves 16 bytes (4 channels)
// per access, lanes run along the channel axis.  All of it is bandwidth-bound; the passes over the full-resolution map z are
// one for the statistics, one for the forward, two for the backward (the per-channel sums, then dz).
//
// No float atomics and no allocation: a sum over all rows of a map goes through the caller's `partials` buffer in the two-stage slab
// scheme of rowsum.h.  The statistics have a finish of their own (Chan's formula on [slab][C][2] partials); the backward's two sums
// are plain ([2][slab][C]) and share their stage 2 with irse_train.hip.  Two runs are bit-identical.
//
// Variance: never E[x^2] - E[x]^2 over the map.  A slab sums (x - K) and (x - K)^2 about a per-channel shift K taken from the DATA
// (the slab's first row), which gives the slab's (count, mean, M2) with a cancellation of the order (mean_slab - K)^2 / var_slab = O(1)
// whatever the offset of the map; stage 2 combines the slabs' triples with Chan's formula.
//
// Data-parallel training: a rank keeps the combine's (mean, M2) of its rows as a record instead of finishing it (gim_bn_stats_record);
// gim_bn_stats_merge combines the ranks' records in rank order with the same formula and the same finish, and the dz pass takes the
// row count of all ranks (gim_bn_pool_bwd_dx_total) with all ranks' sums.
//
// The arg-max of a pooling window is RECOMPUTED in the backward from the four z values (the backward reads z anyway for xhat), not
// stored by the forward.  The affine is applied to each of the four values before the maximum (gamma may be negative); ties go to the
// first maximum in row-major window order, as torch.nn.MaxPool2d.
#include "rowsum.h"

constexpr int BN_FC = 4;              // channels per workgroup of the statistics finish ...
constexpr int BN_FG = 256 / BN_FC;    // ... x 64 groups of at most RS_MAX_SLABS / 64 consecutive slabs

// ---------------------------------------------------------------- statistics, stage 1: (mean, M2) of one slab of rows per channel
__global__ __launch_bounds__(256) void bn_stats_slab_kernel(const float* __restrict__ z, float* __restrict__ partials, long long M, int C,
                                                            long long rps) {
    __shared__ float red[2][RS_HG * RS_CB];
    const int cl = threadIdx.x % RS_CL, hg = threadIdx.x / RS_CL;
    const int c = blockIdx.x * RS_CB + cl * 4;
    const long long r0 = (long long)blockIdx.y * rps;
    const long long r1 = (r0 + rps < M) ? r0 + rps : M;
    const bool ok = c < C;
    f32x4 K = {0.f, 0.f, 0.f, 0.f};
    f32x4 s[2] = {K, K};
    if (ok) {
        K = ld4(z + r0 * C + c);
#pragma unroll 8
        for (long long r = r0 + hg; r < r1; r += RS_HG) {     // (8 independent 16-byte loads in flight per lane)
            const f32x4 d = ld4(z + r * C + c) - K;
            s[0] += d;
            s[1] += d * d;
        }
    }
    group_sum<2>(s, red, cl, hg);
    if (ok && hg == 0) {
        const float inv_n = 1.0f / (float)(r1 - r0);
        float* out = partials + ((long long)blockIdx.y * C + c) * 2;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float m = s[0][e] * inv_n;
            out[2 * e] = K[e] + m;
            out[2 * e + 1] = fmaxf(s[1][e] - s[0][e] * m, 0.f);
        }
    }
}

// ---------------------------------------------------------------- statistics, stage 2: 4 channels x 64 groups of consecutive slabs
// partials hold (mean, M2) of slabs of `rps` rows (the last one shorter), combined with Chan's formula.  Always in the same order: a
// thread combines its group's <= 16 slabs in slab order (their loads are all in flight at once: the partials were just written by
// other CUs, a dependent chain of 64 such loads took longer than stage 1 at the smaller maps), then every eighth thread its 8
// neighbouring groups, then one thread those 8 results.  The running statistics move where given.
struct BnAcc {
    float n, a, b;     // count, mean, M2
};
__device__ __forceinline__ void bn_combine(BnAcc& t, float nb, float pa, float pb) {
    if (nb > 0.f) {
        const float nn = t.n + nb, d = pa - t.a, w = nb / nn;
        t.a += d * w;
        t.b += pb + d * d * (t.n * w);
        t.n = nn;
    }
}
// the combine of one channel's slabs in the order above; all 256 threads call it, the result is valid in the thread it returns true for
// (group 0 of a channel < C)
__device__ __forceinline__ bool bn_combine_slabs(const float* __restrict__ partials, int n_slabs, long long rps, long long M, int C,
                                                 float (*red)[BN_FG * BN_FC], BnAcc& t) {
    const int ci = threadIdx.x % BN_FC, g = threadIdx.x / BN_FC;
    const int c = blockIdx.x * BN_FC + ci;
    const int per = (n_slabs + BN_FG - 1) / BN_FG;      // <= 16
    const int s0 = g * per;
    t = {0.f, 0.f, 0.f};
    if (c < C) {
        float pa[RS_MAX_SLABS / BN_FG], pb[RS_MAX_SLABS / BN_FG];
#pragma unroll
        for (int k = 0; k < RS_MAX_SLABS / BN_FG; ++k) {
            const bool in = k < per && s0 + k < n_slabs;
            const float* p = partials + ((long long)(in ? s0 + k : 0) * C + c) * 2;
            pa[k] = p[0];
            pb[k] = p[1];
        }
#pragma unroll
        for (int k = 0; k < RS_MAX_SLABS / BN_FG; ++k) {
            const long long lo = (long long)(s0 + k) * rps;
            const bool in = k < per && s0 + k < n_slabs;
            const float nb = in ? (float)(((lo + rps < M) ? lo + rps : M) - lo) : 0.f;
            bn_combine(t, nb, in ? pa[k] : 0.f, in ? pb[k] : 0.f);
        }
    }
    red[0][g * BN_FC + ci] = t.n;
    red[1][g * BN_FC + ci] = t.a;
    red[2][g * BN_FC + ci] = t.b;
    __syncthreads();
    if ((g & 7) == 0)
        for (int k = 1; k < 8; ++k) bn_combine(t, red[0][(g + k) * BN_FC + ci], red[1][(g + k) * BN_FC + ci], red[2][(g + k) * BN_FC + ci]);
    __syncthreads();
    if ((g & 7) == 0) {
        red[0][g * BN_FC + ci] = t.n;
        red[1][g * BN_FC + ci] = t.a;
        red[2][g * BN_FC + ci] = t.b;
    }
    __syncthreads();
    if (g != 0 || c >= C) return false;
    for (int k = 8; k < BN_FG; k += 8) bn_combine(t, red[0][k * BN_FC + ci], red[1][k * BN_FC + ci], red[2][k * BN_FC + ci]);
    return true;
}
// the finish of channel c from its (mean a, M2 b) over M rows: shared by the one-process statistics and the merge of several ranks'
__device__ __forceinline__ void bn_finish(int c, float a, float b, long long M, float* __restrict__ mean, float* __restrict__ invstd,
                                          float* __restrict__ running_mean, float* __restrict__ running_var,
                                          long long* __restrict__ nbt, float momentum, float eps) {
    const float var = b / (float)M;
    mean[c] = a;
    invstd[c] = 1.0f / sqrtf(var + eps);
    if (running_mean) {   // the unbiased estimate of the variance
        running_mean[c] = (1.0f - momentum) * running_mean[c] + momentum * a;
        running_var[c] = (1.0f - momentum) * running_var[c] + momentum * (b / (float)(M - 1));
    }
    if (nbt && c == 0) *nbt += 1;
}
__global__ __launch_bounds__(256) void bn_finalize_kernel(const float* __restrict__ partials, int n_slabs, long long rps, long long M, int C,
                                                          float* __restrict__ mean, float* __restrict__ invstd,
                                                          float* __restrict__ running_mean, float* __restrict__ running_var,
                                                          long long* __restrict__ nbt, float momentum, float eps) {
    __shared__ float red[3][BN_FG * BN_FC];
    BnAcc t;
    if (!bn_combine_slabs(partials, n_slabs, rps, M, C, red, t)) return;
    bn_finish(blockIdx.x * BN_FC + threadIdx.x % BN_FC, t.a, t.b, M, mean, invstd, running_mean, running_var, nbt, momentum, eps);
}

// ---------------------------------------------------------------- statistics of one rank among several (data-parallel training)
// the same combine, kept as the rank's record [2][C] = (mean, M2 about that mean) of its M rows instead of being finished
__global__ __launch_bounds__(256) void bn_record_kernel(const float* __restrict__ partials, int n_slabs, long long rps, long long M, int C,
                                                        float* __restrict__ record) {
    __shared__ float red[3][BN_FG * BN_FC];
    BnAcc t;
    if (!bn_combine_slabs(partials, n_slabs, rps, M, C, red, t)) return;
    const int c = blockIdx.x * BN_FC + threadIdx.x % BN_FC;
    record[c] = t.a;
    record[C + c] = t.b;
}
// records [R][2][C] in rank order, n[r] rows each: one thread per channel combines the R triples in rank order (into an empty
// accumulator the first combine is exact: R = 1 gives the bits of bn_finalize_kernel), then the finish over the total row count.
// Every rank that merges the same records gets the same bits.
constexpr int BN_MAX_RANKS = 64;
struct BnCounts {
    long long n[BN_MAX_RANKS];
};
__global__ __launch_bounds__(256) void bn_merge_kernel(const float* __restrict__ records, BnCounts counts, int R, long long M, int C,
                                                       float* __restrict__ mean, float* __restrict__ invstd,
                                                       float* __restrict__ running_mean, float* __restrict__ running_var,
                                                       long long* __restrict__ nbt, float momentum, float eps) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    BnAcc t = {0.f, 0.f, 0.f};
    for (int r = 0; r < R; ++r) bn_combine(t, (float)counts.n[r], records[(long long)(2 * r) * C + c], records[(long long)(2 * r + 1) * C + c]);
    bn_finish(c, t.a, t.b, M, mean, invstd, running_mean, running_var, nbt, momentum, eps);
}

// ---------------------------------------------------------------- stage 2 of the plain sums: out[k][c] = sum over slabs
// grid (ceil(C / 4), sums); 4 channels x 64 slab lanes: a lane adds its slabs lane, lane + 64, ... in that order, then one thread
// per channel the 64 lane sums in lane order.  acc[k] (may be NULL): the total is also ADDED there (a parameter's .grad).
struct RowSums {
    float* out[3];
    float* acc[3];
};
__global__ __launch_bounds__(256) void rowsum_finalize_kernel(const float* __restrict__ partials, int n_slabs, int C, RowSums o) {
    __shared__ float red[64 * 4];
    const int ci = threadIdx.x & 3, lane = threadIdx.x >> 2;
    const int c = blockIdx.x * 4 + ci, k = blockIdx.y;
    float a = 0.f;
    if (c < C) {      // the lane's <= 16 loads all in flight before the first add, as in bn_finalize_kernel
        float p[RS_MAX_SLABS / 64];
#pragma unroll
        for (int j = 0; j < RS_MAX_SLABS / 64; ++j) {
            const int s = lane + 64 * j;
            p[j] = partials[((long long)k * n_slabs + (s < n_slabs ? s : 0)) * C + c];
        }
#pragma unroll
        for (int j = 0; j < RS_MAX_SLABS / 64; ++j)
            if (lane + 64 * j < n_slabs) a += p[j];
    }
    red[lane * 4 + ci] = a;
    __syncthreads();
    if (lane != 0 || c >= C) return;
    float t = 0.f;
    for (int l = 0; l < 64; ++l) t += red[l * 4 + ci];
    o.out[k][c] = t;
    if (o.acc[k]) o.acc[k][c] += t;
}
void rowsum_finalize(const float* partials, int n_slabs, int C, int sums, float* o0, float* o1, float* o2, float* a0, float* a1, float* a2,
                     hipStream_t st) {
    RowSums o = {{o0, o1, o2}, {a0, a1, a2}};
    hipLaunchKernelGGL(rowsum_finalize_kernel, dim3((C + 3) / 4, sums), dim3(256), 0, st, partials, n_slabs, C, o);
}

// ---------------------------------------------------------------- one pooling window of one channel quad
// the four values of the window at zp (rows `row` floats apart, columns C floats), normalised; best / arg: the maximum of the affine
// values and its position 0..3 in row-major order (the first one on a tie)
__device__ __forceinline__ void bn_window(const float* zp, long long row, int C, const BnChan& p, f32x4 (&xh)[4], f32x4& best, int (&arg)[4]) {
    const f32x4 v[4] = {ld4(zp), ld4(zp + C), ld4(zp + row), ld4(zp + row + C)};
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
        const BnChan p = bn_chan<false>(gamma, beta, mean, invstd, nullptr, c);
        f32x4 xh[4], best;
        int arg[4];
        bn_window(z + bn_window_base(i / C4, Ho, Wo, W, C) + c, row, C, p, xh, best, arg);
#pragma unroll
        for (int q = 0; q < 4; ++q) best[q] = fmaxf(best[q], 0.f);
        st4(out + i * 4, best);
    }
}

// ---------------------------------------------------------------- backward, stage 1 of the sums: per slab of POOLED rows
// (sum dyhat, sum dyhat * xhat), dyhat = dp at the window's arg-max where that maximum is > 0
__global__ __launch_bounds__(256) void bn_pool_bwd_slab_kernel(const float* __restrict__ dp, const float* __restrict__ z,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta,
                                                               const float* __restrict__ mean, const float* __restrict__ invstd,
                                                               float* __restrict__ partials, long long Mp, int Ho, int Wo, int C, long long rps) {
    __shared__ float red[2][RS_HG * RS_CB];
    const int cl = threadIdx.x % RS_CL, hg = threadIdx.x / RS_CL;
    const int c = blockIdx.x * RS_CB + cl * 4;
    const int W = Wo * 2;
    const long long row = (long long)W * C;
    const long long r0 = (long long)blockIdx.y * rps;
    const long long r1 = (r0 + rps < Mp) ? r0 + rps : Mp;
    const bool ok = c < C;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 s[2] = {zero, zero};
    if (ok) {
        const BnChan p = bn_chan<false>(gamma, beta, mean, invstd, nullptr, c);
#pragma unroll 2
        for (long long r = r0 + hg; r < r1; r += RS_HG) {
            f32x4 xh[4], best;
            int arg[4];
            const f32x4 g = ld4(dp + r * C + c);
            bn_window(z + bn_window_base(r, Ho, Wo, W, C) + c, row, C, p, xh, best, arg);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float xa = xh[0][q];
#pragma unroll
                for (int k = 1; k < 4; ++k) xa = (arg[q] == k) ? xh[k][q] : xa;
                const float d = best[q] > 0.f ? g[q] : 0.f;
                s[0][q] += d;
                s[1][q] += d * xa;
            }
        }
    }
    group_sum<2>(s, red, cl, hg);
    if (ok && hg == 0) store_partials<2>(s, partials, gridDim.y, blockIdx.y, C, c);
}

// ---------------------------------------------------------------- backward: dz = gamma * invstd * (dyhat - dbeta / M - xhat * dgamma / M)
// M = m_total, the rows dgamma and dbeta were summed over: the map's own 4 Mp, or all ranks' rows with all ranks' sums
__global__ __launch_bounds__(256) void bn_pool_bwd_dx_kernel(const float* __restrict__ dp, const float* __restrict__ z,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             const float* __restrict__ mean, const float* __restrict__ invstd,
                                                             const float* __restrict__ dgamma, const float* __restrict__ dbeta,
                                                             float* __restrict__ dz, long long Mp, int Ho, int Wo, int C, long long m_total) {
    const int C4 = C >> 2, W = Wo * 2;
    const long long n_out = Mp * C4, row = (long long)W * C;
    const float inv_m = 1.0f / (float)m_total;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_out; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % C4) * 4;
        const BnChan p = bn_chan<false>(gamma, beta, mean, invstd, nullptr, c);
        const f32x4 mb = ld4(dbeta + c) * inv_m, mg = ld4(dgamma + c) * inv_m;
        const f32x4 g = ld4(dp + i * 4);
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
        st4(dz + base, o[0]);
        st4(dz + base + C, o[1]);
        st4(dz + base + row, o[2]);
        st4(dz + base + row + C, o[3]);
    }
}

// ---------------------------------------------------------------- da = sign(a - b) * d, db = -da
__global__ __launch_bounds__(256) void absdiff_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ d,
                                                          float* __restrict__ da, float* __restrict__ db, long long n4) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const f32x4 va = ld4(a + i * 4), vb = ld4(b + i * 4), vd = ld4(d + i * 4);
        f32x4 ga, gb;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float t = va[q] - vb[q];
            ga[q] = t > 0.f ? vd[q] : (t < 0.f ? -vd[q] : 0.f);
            gb[q] = -ga[q];
        }
        st4(da + i * 4, ga);
        st4(db + i * 4, gb);
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
    return slab_count(rows);
}

extern "C" int gim_bn_partials_floats(int64_t rows, int C) {
    GIM_CHECK_ARG(rows > 0 && C > 0 && C <= (1 << 18), "bn_partials_floats: bad args");
    return slab_count(rows) * C * 2;
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
    GIM_CHECK_ARG(aligned16(z), "bn_stats: z must be 16-byte aligned");
    GIM_CHECK_ARG(momentum >= 0.f && momentum <= 1.f && eps >= 0.f, "bn_stats: momentum in [0, 1], eps >= 0");
    hipStream_t st = (hipStream_t)stream;
    const long long rps = slab_rows(M);
    const int ns = slab_count(M);
    hipLaunchKernelGGL(bn_stats_slab_kernel, dim3((C + RS_CB - 1) / RS_CB, ns), dim3(256), 0, st, z, partials, (long long)M, C, rps);
    hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + BN_FC - 1) / BN_FC), dim3(256), 0, st, partials, ns, rps, (long long)M, C, mean,
                       invstd, running_mean, running_var, (long long*)num_batches_tracked, momentum, eps);
    return gim_check_launch("gim_bn_stats");
}

extern "C" int gim_bn_stats_record(const float* z, float* partials, float* record, int64_t M, int C, void* stream) {
    GIM_CHECK_ARG(M >= 1 && M < (1ll << 40) && C > 0 && C % 4 == 0 && C <= (1 << 18), "bn_stats_record: bad dims (M >= 1 rows, C % 4 == 0)");
    GIM_CHECK_ARG(z && partials && record, "bn_stats_record: null pointer");
    GIM_CHECK_ARG(aligned16(z), "bn_stats_record: z must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const long long rps = slab_rows(M);
    const int ns = slab_count(M);
    hipLaunchKernelGGL(bn_stats_slab_kernel, dim3((C + RS_CB - 1) / RS_CB, ns), dim3(256), 0, st, z, partials, (long long)M, C, rps);
    hipLaunchKernelGGL(bn_record_kernel, dim3((C + BN_FC - 1) / BN_FC), dim3(256), 0, st, partials, ns, rps, (long long)M, C, record);
    return gim_check_launch("gim_bn_stats_record");
}

extern "C" int gim_bn_stats_merge(const float* records, const int64_t* counts, int R, int C, float* mean, float* invstd,
                                  float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum, float eps,
                                  void* stream) {
    GIM_CHECK_ARG(counts, "bn_stats_merge: null pointer (counts)");      // the sizes are checked before the device pointers
    GIM_CHECK_ARG(R >= 1 && R <= BN_MAX_RANKS, "bn_stats_merge: 1 <= R <= 64 records");
    GIM_CHECK_ARG(C > 0 && C % 4 == 0 && C <= (1 << 18), "bn_stats_merge: bad dims (C % 4 == 0)");
    GIM_CHECK_ARG(!running_mean == !running_var, "bn_stats_merge: running_mean and running_var are given together or not at all");
    GIM_CHECK_ARG(momentum >= 0.f && momentum <= 1.f && eps >= 0.f, "bn_stats_merge: momentum in [0, 1], eps >= 0");
    BnCounts n = {};
    long long total = 0;
    for (int r = 0; r < R; ++r) {
        GIM_CHECK_ARG(counts[r] >= 1 && counts[r] < (1ll << 40), "bn_stats_merge: every rank's row count must be at least 1");
        n.n[r] = counts[r];
        total += counts[r];
    }
    GIM_CHECK_ARG(total >= 2 && total < (1ll << 40), "bn_stats_merge: batch statistics need at least two rows in all");
    GIM_CHECK_ARG(records && mean && invstd, "bn_stats_merge: null pointer");
    hipLaunchKernelGGL(bn_merge_kernel, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream, records, n, R, total, C, mean, invstd,
                       running_mean, running_var, (long long*)num_batches_tracked, momentum, eps);
    return gim_check_launch("gim_bn_stats_merge");
}

extern "C" int gim_bn_relu_maxpool2_fwd(const float* z, const float* gamma, const float* beta, const float* mean, const float* invstd,
                                        float* p, int N, int H, int W, int C, void* stream) {
    GIM_CHECK_ARG(z && gamma && beta && mean && invstd && p, "bn_relu_maxpool2_fwd: null pointer");
    if (bn_check_map("bn_relu_maxpool2_fwd: bad dims (H, W even, C % 4 == 0)", N, H, W, C)) return GIM_E_BADARG;
    GIM_CHECK_ARG(aligned16(z) && aligned16(gamma) && aligned16(beta) && aligned16(mean) && aligned16(invstd) && aligned16(p),
                  "bn_relu_maxpool2_fwd: pointers must be 16-byte aligned");
    const long long Mp = (long long)N * (H / 2) * (W / 2);
    hipLaunchKernelGGL(bn_relu_maxpool2_fwd_kernel, dim3(blocks256(Mp * (C / 4))), dim3(256), 0, (hipStream_t)stream, z, gamma, beta, mean,
                       invstd, p, Mp, H / 2, W / 2, C);
    return gim_check_launch("gim_bn_relu_maxpool2_fwd");
}

extern "C" int gim_bn_pool_bwd_reduce(const float* dp, const float* z, const float* gamma, const float* beta, const float* mean,
                                      const float* invstd, float* partials, float* dgamma, float* dbeta, float* acc_dgamma,
                                      float* acc_dbeta, int N, int H, int W, int C, void* stream) {
    GIM_CHECK_ARG(dp && z && gamma && beta && mean && invstd && partials && dgamma && dbeta, "bn_pool_bwd_reduce: null pointer");
    if (bn_check_map("bn_pool_bwd_reduce: bad dims (H, W even, C % 4 == 0)", N, H, W, C)) return GIM_E_BADARG;
    GIM_CHECK_ARG(aligned16(dp) && aligned16(z) && aligned16(gamma) && aligned16(beta) && aligned16(mean) && aligned16(invstd) &&
                      aligned16(partials), "bn_pool_bwd_reduce: pointers must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const long long Mp = (long long)N * (H / 2) * (W / 2);
    const long long rps = slab_rows(Mp);
    const int ns = slab_count(Mp);
    hipLaunchKernelGGL(bn_pool_bwd_slab_kernel, dim3((C + RS_CB - 1) / RS_CB, ns), dim3(256), 0, st, dp, z, gamma, beta, mean, invstd, partials,
                       Mp, H / 2, W / 2, C, rps);
    rowsum_finalize(partials, ns, C, 2, dbeta, dgamma, nullptr, acc_dbeta, acc_dgamma, nullptr, st);
    return gim_check_launch("gim_bn_pool_bwd_reduce");
}

static int bn_pool_bwd_dx(const char* name, const float* dp, const float* z, const float* gamma, const float* beta, const float* mean,
                          const float* invstd, const float* dgamma, const float* dbeta, float* dz, int N, int H, int W, int C,
                          long long m_total, void* stream) {
    GIM_CHECK_ARG(dp && z && gamma && beta && mean && invstd && dgamma && dbeta && dz, "bn_pool_bwd_dx: null pointer");
    if (bn_check_map("bn_pool_bwd_dx: bad dims (H, W even, C % 4 == 0)", N, H, W, C)) return GIM_E_BADARG;
    GIM_CHECK_ARG(aligned16(dp) && aligned16(z) && aligned16(gamma) && aligned16(beta) && aligned16(mean) && aligned16(invstd) &&
                      aligned16(dgamma) && aligned16(dbeta) && aligned16(dz),
                  "bn_pool_bwd_dx: pointers must be 16-byte aligned");
    const long long Mp = (long long)N * (H / 2) * (W / 2);
    hipLaunchKernelGGL(bn_pool_bwd_dx_kernel, dim3(blocks256(Mp * (C / 4))), dim3(256), 0, (hipStream_t)stream, dp, z, gamma, beta, mean, invstd,
                       dgamma, dbeta, dz, Mp, H / 2, W / 2, C, m_total);
    return gim_check_launch(name);
}

extern "C" int gim_bn_pool_bwd_dx(const float* dp, const float* z, const float* gamma, const float* beta, const float* mean,
                                  const float* invstd, const float* dgamma, const float* dbeta, float* dz, int N, int H, int W, int C,
                                  void* stream) {
    return bn_pool_bwd_dx("gim_bn_pool_bwd_dx", dp, z, gamma, beta, mean, invstd, dgamma, dbeta, dz, N, H, W, C,
                          4ll * N * (H / 2) * (W / 2), stream);      // (bad dims are refused before the count is read)
}

extern "C" int gim_bn_pool_bwd_dx_total(const float* dp, const float* z, const float* gamma, const float* beta, const float* mean,
                                        const float* invstd, const float* dgamma, const float* dbeta, float* dz, int N, int H, int W,
                                        int C, int64_t M_total, void* stream) {
    GIM_CHECK_ARG(M_total >= 4ll * N * (H / 2) * (W / 2) && M_total < (1ll << 40),
                  "bn_pool_bwd_dx_total: M_total must be at least the map's own N * H * W rows");
    return bn_pool_bwd_dx("gim_bn_pool_bwd_dx_total", dp, z, gamma, beta, mean, invstd, dgamma, dbeta, dz, N, H, W, C, (long long)M_total,
                          stream);
}

extern "C" int gim_absdiff_bwd(const float* a, const float* b, const float* d, float* da, float* db, int64_t n, void* stream) {
    GIM_CHECK_ARG(a && b && d && da && db && n > 0 && n % 4 == 0, "absdiff_bwd: bad args (n % 4 == 0)");
    GIM_CHECK_ARG(aligned16(a) && aligned16(b) && aligned16(d) && aligned16(da) && aligned16(db),
                  "absdiff_bwd: pointers must be 16-byte aligned");
    hipLaunchKernelGGL(absdiff_bwd_kernel, dim3(blocks256(n / 4)), dim3(256), 0, (hipStream_t)stream, a, b, d, da, db, (long long)(n / 4));
    return gim_check_launch("gim_absdiff_bwd");
}

extern "C" int gim_logit_accuracy(const float* logits, int n_pos, int n, float* out, void* stream) {
    GIM_CHECK_ARG(logits && out && n > 0 && n_pos >= 0 && n_pos <= n && n < (1 << 24), "logit_accuracy: bad args");
    hipLaunchKernelGGL(logit_accuracy_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, logits, n_pos, n, out);
    return gim_check_launch("gim_logit_accuracy");
}
