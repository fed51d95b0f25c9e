// Spectral-norm power iteration and the weight-gradient finish (HBM-bound GEMV-shaped work).
//
// Weight W is [Cout][T][Cin] in memory (T = KH*KH taps); torch's weight_mat is [Cout][Cin*T] with
// column q = ci*T + tap.  u is [Cout]; v is [Cin*T] in torch's order, so the kernels translate
// physical column p = tap*Cin + ci  <->  q = ci*T + tap.
#include "common.h"

#define SN_R 8  // row chunks of the W^T u partial sums

// -------------------------------------------------------------------------------------------------
// power iteration: four stages over a view of ONE weight.  The per-call kernels (sn_*) get the view by value; the batched ones
// (snb_*) build it from their job, so one round of every conv of a model is 4 launches: the iterations are data independent
// and a model runs all its rounds up front instead of 4 tiny launches per conv call.
// -------------------------------------------------------------------------------------------------
struct SnView {
    const float* w;
    float *u, *v;                  // state, updated in place when training
    float *sigma, *u_out, *v_out;  // results: copies of the vectors used
    float *part, *v_phys, *tvec;   // scratch: [SN_R][K], [K] (v in physical order), [Cout]
    int Cout, Cin, T, K;
};

__host__ __device__ __forceinline__ SnView sn_view(const float* w, float* u, float* v, float* sigma, float* u_out, float* v_out,
                                                   float* scratch, int Cout, int Cin, int KH) {
    SnView s;
    s.w = w; s.u = u; s.v = v; s.sigma = sigma; s.u_out = u_out; s.v_out = v_out;
    s.Cout = Cout; s.Cin = Cin; s.T = KH * KH; s.K = Cin * s.T;
    s.part = scratch;
    s.v_phys = scratch + (long long)SN_R * s.K;
    s.tvec = s.v_phys + s.K;
    return s;
}
__device__ __forceinline__ SnView sn_view(const gim_sn_job& jb, float* out_base) {
    return sn_view(jb.w, jb.u, jb.v, out_base + jb.off_sigma, out_base + jb.off_u, out_base + jb.off_v, out_base + jb.off_scratch,
                   jb.Cout, jb.Cin, jb.KH);
}
__host__ __device__ __forceinline__ int sn_row_chunks(int Cout) { return min(SN_R, (Cout + 63) / 64); }

// part[r][p] = sum over the r-th chunk of rows co of W[co][p] * u[co]
__device__ __forceinline__ void sn_colpart(const SnView& s, int p, int r, int rows_per) {
    if (p >= s.K) return;
    const int c0 = r * rows_per, c1 = min(s.Cout, c0 + rows_per);
    float acc = 0.f;
    for (int co = c0; co < c1; ++co) acc += s.w[(long long)co * s.K + p] * s.u[co];
    s.part[(long long)r * s.K + p] = acc;
}

// single block of NT threads.  training: a = sum_r part[r]; v = a / max(|a|, eps) ; else v given.
// writes v_phys (physical order, scratch), v (torch order, in place when training) and v_out (copy).
template <int NT>
__device__ __forceinline__ void sn_vnorm(const SnView& s, int training, float* red) {
    if (training) {
        const int R = sn_row_chunks(s.Cout);
        float ss = 0.f;
        for (int p = threadIdx.x; p < s.K; p += NT) {
            float a = 0.f;
            for (int r = 0; r < R; ++r) a += s.part[(long long)r * s.K + p];
            s.v_phys[p] = a;
            ss += a * a;
        }
        const float inv = 1.0f / fmaxf(sqrtf(block_sum<NT>(ss, red)), 1e-12f);
        for (int p = threadIdx.x; p < s.K; p += NT) {   // each thread re-reads only what it wrote itself
            const float val = s.v_phys[p] * inv;
            const int tap = p / s.Cin, ci = p - tap * s.Cin;
            const int q = ci * s.T + tap;
            s.v_phys[p] = val;
            s.v[q] = val;
            s.v_out[q] = val;
        }
    } else {
        for (int q = threadIdx.x; q < s.K; q += NT) {
            const int ci = q / s.T, tap = q - ci * s.T;
            const float val = s.v[q];
            s.v_phys[tap * s.Cin + ci] = val;
            s.v_out[q] = val;
        }
    }
}

// t[co] = sum_p W[co][p] * v_phys[p]; one wave per row
__device__ __forceinline__ void sn_rowdot(const SnView& s, int co, int lane) {
    if (co >= s.Cout) return;
    const float* row = s.w + (long long)co * s.K;
    float acc = 0.f;
    for (int p = lane; p < s.K; p += 64) acc += row[p] * s.v_phys[p];
    acc = wave_sum(acc);
    if (lane == 0) s.tvec[co] = acc;
}

// single block of 256. training: u = t / max(|t|, eps); sigma = u . t ; else sigma = u . t with the stored u.
__device__ __forceinline__ void sn_final(const SnView& s, int training, float* red) {
    float inv = 0.f;
    if (training) {
        float ss = 0.f;
        for (int c = threadIdx.x; c < s.Cout; c += 256) ss += s.tvec[c] * s.tvec[c];
        inv = 1.0f / fmaxf(sqrtf(block_sum_256(ss, red)), 1e-12f);
    }
    float dot = 0.f;
    for (int c = threadIdx.x; c < s.Cout; c += 256) {
        float uv;
        if (training) {
            uv = s.tvec[c] * inv;
            s.u[c] = uv;
        } else {
            uv = s.u[c];
        }
        s.u_out[c] = uv;
        dot += uv * s.tvec[c];
    }
    dot = block_sum_256(dot, red);
    if (threadIdx.x == 0) s.sigma[0] = dot;
}

__global__ __launch_bounds__(256) void sn_colpart_kernel(const SnView s, int rows_per) {
    sn_colpart(s, blockIdx.x * 256 + threadIdx.x, blockIdx.y, rows_per);
}
__global__ __launch_bounds__(256) void sn_rowdot_kernel(const SnView s) {
    sn_rowdot(s, blockIdx.x * 4 + (threadIdx.x >> 6), threadIdx.x & 63);
}
// (the four vectors once more as arguments of their own: __restrict__ holds on kernel arguments only, and with it the compiler
//  keeps the unrolled store loop this kernel always had; without, + 5 % on the entry at 512 x 512 x 3 x 3)
__global__ __launch_bounds__(256) void sn_vnorm_kernel(SnView s, float* __restrict__ part, float* __restrict__ v_phys,
                                                       float* __restrict__ v, float* __restrict__ v_out, int training) {
    __shared__ float red[4];
    s.part = part; s.v_phys = v_phys; s.v = v; s.v_out = v_out;
    sn_vnorm<256>(s, training, red);
}
__global__ __launch_bounds__(256) void sn_final_kernel(const SnView s, int training) {
    __shared__ float red[4];
    sn_final(s, training, red);
}

extern "C" int gim_spectral_sigma(const float* w, float* u, float* v, float* sigma, float* u_out, float* v_out, float* scratch,
                                  int Cout, int Cin, int KH, int training, void* stream) {
    GIM_CHECK_ARG(w && u && v && sigma && u_out && v_out && scratch, "spectral_sigma: null pointer");
    GIM_CHECK_ARG(Cout > 0 && Cin > 0 && KH > 0, "spectral_sigma: bad dims");
    hipStream_t st = (hipStream_t)stream;
    const SnView s = sn_view(w, u, v, sigma, u_out, v_out, scratch, Cout, Cin, KH);
    if (training) {
        const int R = sn_row_chunks(Cout);
        hipLaunchKernelGGL(sn_colpart_kernel, dim3((s.K + 255) / 256, R), dim3(256), 0, st, s, (Cout + R - 1) / R);
    }
    hipLaunchKernelGGL(sn_vnorm_kernel, dim3(1), dim3(256), 0, st, s, s.part, s.v_phys, s.v, s.v_out, training);
    hipLaunchKernelGGL(sn_rowdot_kernel, dim3((Cout + 3) / 4), dim3(256), 0, st, s);
    hipLaunchKernelGGL(sn_final_kernel, dim3(1), dim3(256), 0, st, s, training);
    return gim_check_launch("gim_spectral_sigma");
}

// Batched form.  Job table and block->job maps are static per model; per-round outputs live at static offsets from `out_base`.
__global__ __launch_bounds__(256) void snb_colpart_kernel(const gim_sn_job* __restrict__ jobs, const int4* __restrict__ tab,
                                                          float* __restrict__ out_base) {
    const int4 e = tab[blockIdx.x];  // {job, column block, row chunk, rows per chunk}
    sn_colpart(sn_view(jobs[e.x], out_base), e.y * 256 + threadIdx.x, e.z, e.w);
}

// One block of 1024 threads per job (the jobs are few - one per conv - and a 256-thread block walking the 4608-5120 columns of
// the largest ones was a 46 us chain of dependent-latency loads at the head of every forward pass).
__global__ __launch_bounds__(1024) void snb_vnorm_kernel(const gim_sn_job* __restrict__ jobs, float* __restrict__ out_base, int training) {
    __shared__ float red[16];
    sn_vnorm<1024>(sn_view(jobs[blockIdx.x], out_base), training, red);
}

__global__ __launch_bounds__(256) void snb_rowdot_kernel(const gim_sn_job* __restrict__ jobs, const int2* __restrict__ tab,
                                                         float* __restrict__ out_base) {
    const int2 e = tab[blockIdx.x];  // {job, row block}
    sn_rowdot(sn_view(jobs[e.x], out_base), e.y * 4 + (threadIdx.x >> 6), threadIdx.x & 63);
}

__global__ __launch_bounds__(256) void snb_final_kernel(const gim_sn_job* __restrict__ jobs, float* __restrict__ out_base, int training) {
    __shared__ float red[4];
    sn_final(sn_view(jobs[blockIdx.x], out_base), training, red);
}

extern "C" int gim_spectral_sigma_batched(const gim_sn_job* jobs, int n_jobs, const int32_t* tab_cols, int n_col_blocks,
                                          const int32_t* tab_rows, int n_row_blocks, float* out_base, int training, void* stream) {
    GIM_CHECK_ARG(jobs && n_jobs > 0 && tab_cols && tab_rows && out_base && n_col_blocks > 0 && n_row_blocks > 0,
                  "spectral_sigma_batched: bad args");
    hipStream_t st = (hipStream_t)stream;
    if (training)
        hipLaunchKernelGGL(snb_colpart_kernel, dim3(n_col_blocks), dim3(256), 0, st, jobs, reinterpret_cast<const int4*>(tab_cols), out_base);
    hipLaunchKernelGGL(snb_vnorm_kernel, dim3(n_jobs), dim3(1024), 0, st, jobs, out_base, training);
    hipLaunchKernelGGL(snb_rowdot_kernel, dim3(n_row_blocks), dim3(256), 0, st, jobs, reinterpret_cast<const int2*>(tab_rows), out_base);
    hipLaunchKernelGGL(snb_final_kernel, dim3(n_jobs), dim3(256), 0, st, jobs, out_base, training);
    return gim_check_launch("gim_spectral_sigma_batched");
}

// -------------------------------------------------------------------------------------------------
// weight-gradient finish
// -------------------------------------------------------------------------------------------------
#define WF_BLOCKS 512

// dw[i] = sum_s slabs[s][i] (+ <dw, w> partials, + bias sums).  64 elements x 4 slab groups per block pass: the
// slab loop of one element is spread over 4 threads and unrolled, so a 100-slab reduction keeps ~32 independent
// loads in flight per element instead of one dependent chain.
__global__ __launch_bounds__(256) void wgrad_sum_kernel(const float* __restrict__ slabs, int n_slabs, long long n,
                                                        const float* __restrict__ w, float* __restrict__ dw,
                                                        float* __restrict__ partial, const float* __restrict__ bias_slabs,
                                                        float* __restrict__ db, int Cout, int acc_dw, int acc_db) {
    __shared__ float red[4];
    __shared__ float part[4][64];
    float dot = 0.f;
    if (db) {
        for (int c = blockIdx.x * 256 + threadIdx.x; c < Cout; c += gridDim.x * 256) {
            float g = acc_db ? db[c] : 0.f;
            for (int s = 0; s < n_slabs; ++s) g += bias_slabs[(long long)s * Cout + c];
            db[c] = g;
        }
    }
    const int el = threadIdx.x & 63, sg = threadIdx.x >> 6;
    for (long long i0 = (long long)blockIdx.x * 64; i0 < n; i0 += (long long)gridDim.x * 64) {
        const long long i = i0 + el;
        float g = 0.f;
        if (i < n) {
            int s = sg;
#pragma unroll 1
            for (; s + 12 < n_slabs; s += 16) {
                const float g0 = slabs[(long long)s * n + i], g1 = slabs[(long long)(s + 4) * n + i];
                const float g2 = slabs[(long long)(s + 8) * n + i], g3 = slabs[(long long)(s + 12) * n + i];
                g += (g0 + g1) + (g2 + g3);
            }
            for (; s < n_slabs; s += 4) g += slabs[(long long)s * n + i];
        }
        part[sg][el] = g;
        __syncthreads();
        if (sg == 0 && i < n) {
            g = (part[0][el] + part[1][el]) + (part[2][el] + part[3][el]);
            dw[i] = acc_dw ? dw[i] + g : g;
            if (w) dot += g * w[i];
        }
        __syncthreads();
    }
    if (partial) {
        dot = block_sum_256(dot, red);
        if (threadIdx.x == 0) partial[blockIdx.x] = dot;
    }
}

// The two bodies below are shared by the per-call finish (gim_wgrad_finish, slab mode) and the batched one (wgq_*, the training
// step).  All their index arithmetic is 32-bit - Cout*(K+1)^2*Cin < 2^31 per weight, checked by gim_wgrad_finish and by
// ops.WgradQueue for the job tables: the first version's 64-bit divisions per element made these HBM-bound passes 3x slower
// than the bytes they move.

// Where tap (a, b) of dF[co][a][b][ci], the gradient of the folded weights [Cout][K+1][K+1][Cin], lies in the source:
//   fold 1: src = dF itself;   fold 2: src = G [Cin][K+1][K+1][Cout] with dF[co][a][b][ci] = G[ci][K-a][K-b][co]
__device__ __forceinline__ unsigned fold_index(unsigned co, unsigned a, unsigned b, unsigned ci, unsigned Cout, unsigned Cin,
                                               unsigned K, int fold) {
    const unsigned KF = K + 1;
    return fold == 1 ? ((co * KF + a) * KF + b) * Cin + ci : ((ci * KF + (K - a)) * KF + (K - b)) * Cout + co;
}

// element i of the un-folded gradient [Cout][K][K][Cin]:
//   fold 0: src[i];   fold 1: dW[co][kh][kw][ci] = 0.25 * sum_{dh,dw} dF[co][kh+dh][kw+dw][ci];   fold 2: the same sum without the
//   factor;   fold 3: the row-padded slot of gim_conv2d_wgrad_rows_acc, [Cout][K][K * Cin rounded up to 16]
__device__ __forceinline__ float unfold_load(const float* __restrict__ src, unsigned i, unsigned Cout, unsigned Cin, unsigned K, int fold) {
    if (fold == 0) return src[i];
    const unsigned r1 = i / Cin, ci = i - r1 * Cin;
    const unsigned r2 = r1 / K, kw = r1 - r2 * K;
    if (fold == 3) return src[r2 * ((K * Cin + 15u) & ~15u) + kw * Cin + ci];
    const unsigned co = r2 / K, kh = r2 - co * K;
    float g = 0.f;
#pragma unroll
    for (unsigned dh = 0; dh < 2; ++dh)
#pragma unroll
        for (unsigned dwd = 0; dwd < 2; ++dwd) g += src[fold_index(co, kh + dh, kw + dwd, ci, Cout, Cin, K, fold)];
    return fold == 1 ? 0.25f * g : g;
}

// Spectral-norm chain rule dW = g / sigma - (<g, W> / sigma^2) u v^T for NV consecutive input channels of one (co, tap), with
// inv = 1 / sigma and coef = <g, W> / sigma^2:  out[e] = g[e] * inv - (coef * u[co]) * v[(ci + e) * T + tap].
// The element is (co, p = tap * Cin + ci); p may run past Kc = T * Cin (whole output channels are carried into co: a chunk
// states the (co, p) of its first element once and adds the offset, so only layers with fewer weights per output channel than
// the chunk wrap more than once) and ONE division by Cin is left per element.
template <int NV>
__device__ __forceinline__ void sn_chain(const float* g, float* out, float inv, float coef, const float* __restrict__ u,
                                         const float* __restrict__ v, unsigned co, unsigned p, unsigned Kc, unsigned Cin, unsigned T) {
    if (p >= Kc) {
        const unsigned q = p / Kc;
        co += q;
        p -= q * Kc;
    }
    const unsigned tap = p / Cin, ci = p - tap * Cin;
    const float cu = coef * u[co];
    const float* vq = v + ci * T + tap;
#pragma unroll
    for (int e = 0; e < NV; ++e) out[e] = g[e] * inv - cu * vq[e * T];
}

__global__ __launch_bounds__(256) void wgrad_unfold_kernel(const float* __restrict__ src, const float* __restrict__ w,
                                                           float* __restrict__ dw, float* __restrict__ partial, int Cout, int Cin,
                                                           int K, int fold) {
    __shared__ float red[4];
    const unsigned n = (unsigned)Cout * K * K * Cin;
    float dot = 0.f;
    for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const float g = unfold_load(src, i, Cout, Cin, K, fold);
        dw[i] = g;
        if (w) dot += g * w[i];
    }
    if (partial) {
        dot = block_sum_256(dot, red);
        if (threadIdx.x == 0) partial[blockIdx.x] = dot;
    }
}

__global__ __launch_bounds__(256) void wgrad_sn_apply_kernel(const float* __restrict__ g, float* __restrict__ dw, int accumulate,
                                                             const float* __restrict__ partial, int n_part,
                                                             const float* __restrict__ sigma, const float* __restrict__ u,
                                                             const float* __restrict__ v, unsigned n, int Cin, int T) {
    __shared__ float red[4];
    float d = 0.f;
    for (int i = threadIdx.x; i < n_part; i += 256) d += partial[i];
    d = block_sum_256(d, red);
    const float inv = 1.0f / sigma[0];
    const float coef = d * inv * inv;
    for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        float val;
        sn_chain<1>(g + i, &val, inv, coef, u, v, 0, i, Cin * T, Cin, T);
        dw[i] = accumulate ? dw[i] + val : val;
    }
}

extern "C" int gim_wgrad_finish(const float* slabs, const float* bias_slabs, int n_slabs, const float* w, const float* sigma,
                                const float* u, const float* v, float* dw, float* db, float* scratch, int Cout, int Cin, int KH,
                                int fold, float* acc_dw, float* acc_db, void* stream) {
    GIM_CHECK_ARG(slabs && dw && n_slabs > 0, "wgrad_finish: bad args");
    GIM_CHECK_ARG((!db && !acc_db) || bias_slabs, "wgrad_finish: db needs bias_slabs");
    GIM_CHECK_ARG(!sigma || (w && u && v && scratch), "wgrad_finish: spectral form needs w, u, v, scratch");
    GIM_CHECK_ARG(fold >= 0 && fold <= 2 && (!fold || scratch), "wgrad_finish: bad fold / missing scratch");
    hipStream_t st = (hipStream_t)stream;
    const int T = KH * KH;
    const long long n = (long long)Cout * Cin * T;
    const long long nf = (long long)Cout * Cin * (KH + 1) * (KH + 1);   // the folded layout
    GIM_CHECK_ARG(nf < (1LL << 31), "wgrad_finish: Cout*(KH+1)^2*Cin must be below 2^31");
    int blocks = (int)((n + 1023) / 1024);
    if (blocks > WF_BLOCKS) blocks = WF_BLOCKS;
    if (blocks < 1) blocks = 1;
    int sblocks = (int)((n + 63) / 64);  // wgrad_sum_kernel: 64 elements per block pass
    if (sblocks > WF_BLOCKS) sblocks = WF_BLOCKS;
    float* bias_out = acc_db ? acc_db : db;
    const int bias_acc = acc_db ? 1 : 0;
    // the plain (no sigma, no fold) form can sum straight into the accumulation target
    const bool direct = !sigma && !fold && acc_dw;
    if (fold == 0) {
        hipLaunchKernelGGL(wgrad_sum_kernel, dim3(sblocks), dim3(256), 0, st, slabs, n_slabs, n, sigma ? w : nullptr,
                           direct ? acc_dw : dw, sigma ? scratch : nullptr, bias_slabs, bias_out, Cout, direct ? 1 : 0, bias_acc);
        blocks = sblocks;  // number of <g, w> partials for the spectral apply
    } else {
        // 1) sum the slabs (folded layout) into scratch[512 ...], bias on the way; 2) un-fold into dw (+ <g, w>)
        float* fsum = scratch + WF_BLOCKS;
        int fb = (int)((nf + 63) / 64);
        if (fb > WF_BLOCKS) fb = WF_BLOCKS;
        hipLaunchKernelGGL(wgrad_sum_kernel, dim3(fb), dim3(256), 0, st, slabs, n_slabs, nf, (const float*)nullptr, fsum,
                           (float*)nullptr, bias_slabs, bias_out, Cout, 0, bias_acc);
        hipLaunchKernelGGL(wgrad_unfold_kernel, dim3(blocks), dim3(256), 0, st, fsum, sigma ? w : nullptr, dw,
                           sigma ? scratch : nullptr, Cout, Cin, KH, fold);
    }
    if (sigma) {
        hipLaunchKernelGGL(wgrad_sn_apply_kernel, dim3(blocks), dim3(256), 0, st, dw, acc_dw ? acc_dw : dw, acc_dw ? 1 : 0, scratch,
                           blocks, sigma, u, v, (unsigned)n, Cin, T);
    } else if (acc_dw && !direct) {
        GIM_CHECK_ARG(false, "wgrad_finish: acc_dw without sigma is only supported for fold == 0");
    }
    return gim_check_launch("gim_wgrad_finish");
}

// -------------------------------------------------------------------------------------------------
// batched weight-gradient finish: every conv / linear of one backward pass in TWO launches.
// Each job's raw gradient was accumulated (float atomics) into a pre-zeroed arena slot by gim_conv2d_wgrad_acc; here it is
// un-folded (pool / sub-pixel forms), pushed through the spectral-norm chain rule and ADDED into the optimizer's flat
// gradient bucket.  One block handles WGQ_CHUNK elements of one job (table built on the host, static per model).
// -------------------------------------------------------------------------------------------------
#define WGQ_CHUNK 4096

__device__ __forceinline__ bool wgq_aligned16(const void* a, const void* b, const void* c) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}

__global__ __launch_bounds__(256) void wgq_reduce_kernel(const gim_wgrad_job* __restrict__ jobs, const int2* __restrict__ tab) {
    __shared__ float red[4];
    const int2 e = tab[blockIdx.x];  // {job, chunk}
    const gim_wgrad_job jb = jobs[e.x];
    const unsigned n = (unsigned)jb.Cout * jb.K * jb.K * jb.Cin;
    const unsigned i0 = (unsigned)e.y * WGQ_CHUNK;
    const unsigned cnt = min((unsigned)WGQ_CHUNK, n - i0);
    const bool sn = jb.sigma != nullptr;
    float dot = 0.f;
    if (sn && jb.fold == 2 && (jb.Cout & 63) == 0 && (jb.Cin & 63) == 0) {
        // Sub-pixel (role-swapped) jobs hold G[ci][KF][KF][co]; the gradient wants [co][K][K][ci].  Read by flat output index,
        // consecutive lanes (ci) are KF*KF*Cout floats apart in G - one 64-byte sector per lane and load.  Instead this block takes
        // a 64 co x 64 ci tile of ONE tap (the chunk id is re-read as (co tile, ci tile, tap): the same 4096 elements per block,
        // every element covered once, so `partial` and `tmp` keep their meaning), reads G along co, turns the tile in LDS and
        // writes along ci.
        __shared__ float tile[64][65];
        const unsigned K = jb.K, T = K * K, Cin = jb.Cin, Cout = jb.Cout, tiles_ci = Cin >> 6;
        const unsigned tap = (unsigned)e.y % T, r = (unsigned)e.y / T;
        const unsigned ci0 = (r % tiles_ci) << 6, co0 = (r / tiles_ci) << 6;
        const unsigned kh = tap / K, kw = tap - kh * K;
        const unsigned lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll 4
        for (unsigned j = 0; j < 16; ++j) {
            const unsigned ci = ci0 + wv + 4 * j, co = co0 + lane;
            const float* s = jb.src;
            tile[wv + 4 * j][lane] = (s[fold_index(co, kh, kw, ci, Cout, Cin, K, 2)] + s[fold_index(co, kh, kw + 1, ci, Cout, Cin, K, 2)]) +
                                     (s[fold_index(co, kh + 1, kw, ci, Cout, Cin, K, 2)] + s[fold_index(co, kh + 1, kw + 1, ci, Cout, Cin, K, 2)]);
        }
        __syncthreads();
#pragma unroll 4
        for (unsigned j = 0; j < 16; ++j) {
            const unsigned co = co0 + wv + 4 * j;
            const float g = tile[lane][wv + 4 * j];
            const unsigned i = ((co * K + kh) * K + kw) * Cin + ci0 + lane;
            jb.tmp[i] = g;
            dot += g * jb.w[i];
        }
    } else if (sn && jb.fold == 0 && (n & 3) == 0 && wgq_aligned16(jb.src, jb.w, jb.w)) {
        // <G, W> only (the apply kernel reads G again): 16-byte loads
        for (unsigned t = threadIdx.x * 4; t < cnt; t += 1024) {
            const float4 g = *reinterpret_cast<const float4*>(jb.src + i0 + t);
            const float4 w = *reinterpret_cast<const float4*>(jb.w + i0 + t);
            dot += g.x * w.x + g.y * w.y + g.z * w.z + g.w * w.w;
        }
    } else if (!sn && jb.fold == 0 && jb.exclusive && (n & 3) == 0 && wgq_aligned16(jb.src, jb.grad_w, jb.grad_w)) {
        // the only job of this gradient in the pass: plain 16-byte read-modify-write instead of float atomics
        for (unsigned t = threadIdx.x * 4; t < cnt; t += 1024) {
            const float4 g = *reinterpret_cast<const float4*>(jb.src + i0 + t);
            float4* dst = reinterpret_cast<float4*>(jb.grad_w + i0 + t);
            float4 o = *dst;
            o.x += g.x; o.y += g.y; o.z += g.z; o.w += g.w;
            *dst = o;
        }
    } else {
        // lane-consecutive elements: the float atomics of a wave then hit 256 consecutive bytes (4 elements per lane made every
        // atomic instruction span 1 KB and the pass 1.4x slower than the scalar form)
#pragma unroll 4
        for (unsigned t = threadIdx.x; t < cnt; t += 256) {
            const unsigned i = i0 + t;
            const float g = unfold_load(jb.src, i, jb.Cout, jb.Cin, jb.K, jb.fold);
            if (sn) {
                if (jb.fold) jb.tmp[i] = g;
                dot += g * jb.w[i];
            } else {   // several jobs (calls of the same conv) may target one gradient
                atomicAdd(&jb.grad_w[i], g);
            }
        }
    }
    if (sn) {
        dot = block_sum_256(dot, red);
        if (threadIdx.x == 0) jb.partial[e.y] = dot;
    }
    if (e.y == 0 && jb.bias_src)
        for (int c = threadIdx.x; c < jb.Cout; c += 256) atomicAdd(&jb.grad_b[c], jb.bias_src[c]);
}

__global__ __launch_bounds__(256) void wgq_apply_kernel(const gim_wgrad_job* __restrict__ jobs, const int2* __restrict__ tab) {
    __shared__ float red[4];
    const int2 e = tab[blockIdx.x];
    const gim_wgrad_job jb = jobs[e.x];
    float d = 0.f;
    for (int i = threadIdx.x; i < jb.n_chunks; i += 256) d += jb.partial[i];
    d = block_sum_256(d, red);
    const float inv = 1.0f / jb.sigma[0];
    const float coef = d * inv * inv;
    const unsigned Cin = jb.Cin, T = (unsigned)jb.K * jb.K, Kc = Cin * T;
    const unsigned n = (unsigned)jb.Cout * Kc;
    const unsigned i0 = (unsigned)e.y * WGQ_CHUNK;
    const unsigned cnt = min((unsigned)WGQ_CHUNK, n - i0);
    const float* __restrict__ g = jb.fold ? jb.tmp : jb.src;
    const unsigned co0 = i0 / Kc, p0 = i0 - co0 * Kc;   // (co, p) of the chunk's first element, once per block
    if (jb.exclusive && (Cin & 3) == 0 && wgq_aligned16(g, jb.grad_w, jb.grad_w)) {
        // the only job of this gradient in the pass: 16-byte read-modify-write (4 consecutive input channels share the output
        // channel and the tap)
        for (unsigned t = threadIdx.x * 4; t < cnt; t += 1024) {
            const float4 gv = *reinterpret_cast<const float4*>(g + i0 + t);
            const float ge[4] = {gv.x, gv.y, gv.z, gv.w};
            float val[4];
            sn_chain<4>(ge, val, inv, coef, jb.u, jb.v, co0, p0 + t, Kc, Cin, T);
            float4* dst = reinterpret_cast<float4*>(jb.grad_w + i0 + t);
            float4 o = *dst;
            o.x += val[0]; o.y += val[1]; o.z += val[2]; o.w += val[3];
            *dst = o;
        }
        return;
    }
#pragma unroll 4
    for (unsigned t = threadIdx.x; t < cnt; t += 256) {
        float val;
        sn_chain<1>(g + i0 + t, &val, inv, coef, jb.u, jb.v, co0, p0 + t, Kc, Cin, T);
        atomicAdd(&jb.grad_w[i0 + t], val);
    }
}

extern "C" int gim_wgrad_finish_batched(const gim_wgrad_job* jobs, int n_jobs, const int32_t* tab, int n_blocks,
                                        const int32_t* tab_sn, int n_blocks_sn, void* stream) {
    GIM_CHECK_ARG(jobs && n_jobs > 0 && tab && n_blocks > 0 && n_blocks_sn >= 0 && (tab_sn || n_blocks_sn == 0),
                  "wgrad_finish_batched: bad args");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(wgq_reduce_kernel, dim3(n_blocks), dim3(256), 0, st, jobs, reinterpret_cast<const int2*>(tab));
    if (n_blocks_sn > 0)
        hipLaunchKernelGGL(wgq_apply_kernel, dim3(n_blocks_sn), dim3(256), 0, st, jobs, reinterpret_cast<const int2*>(tab_sn));
    return gim_check_launch("gim_wgrad_finish_batched");
}
