// ROC statistics of two score sets as exact integer counts (authentication_eval.roc_statistics): for every candidate threshold c
// the number of positives >= c, of negatives < c and of negatives == c - no sort, no float atomics, nothing rounded.
//
// Counts launch: one thread per candidate (its three counters live in registers), 256 candidates per workgroup.  The scores go
// through LDS in tiles of ROC_TILE floats: thread t fetches the 16-byte quad t of the tile (coalesced; the quads are taken from the
// 16-byte-aligned address at or below the array's start, so any float pointer is accepted and a quad that sticks out at either
// end is loaded element-wise), then every lane reads the SAME quad of the tile per step (one broadcast ds_read_b128, conflict-
// free) and compares its candidate with the four scores.  The unused elements of a tile hold NaN: a NaN compares false in all
// three tests, so the inner loop needs no bounds, and a NaN among the scores or candidates counts nowhere, as IEEE says.
// With few candidates and many scores grid.y cuts the tiles (positives first, then negatives) into gim_roc_slices() slices of
// whole tiles; slices combine by integer atomicAdd into counts that the entry point zeroes first on the same stream - integer
// addition commutes, so the counts are bit-identical between runs and do not depend on the slicing.
//
// Finish launch (gim_roc_calibrate): ONE workgroup loops over the candidates [pos; neg], keeps per thread the two AUC sums, the
// NaN count and the best (key, value, index) and folds them through LDS.  The order "larger key, then larger value, then
// smaller index" is total, so the fold's shape does not matter either.
#include "common.h"

constexpr int ROC_TILE = 1024;        // floats of one LDS tile = 256 threads x one 16-byte quad (tests/test_gpu_roc.py states it)
constexpr int ROC_THREADS = 256;
// workgroups a launch aims at before it stops slicing the scores: 16 per CU.  Measured on 100 000 + 100 000 scores as candidates
// (782 workgroups of candidates): 4.80 ms unsliced (3 waves per SIMD, and 3 or 4 workgroups on a CU), 3.68 ms at a target of 2048,
// 3.29 ms at 4096 (6 slices)
constexpr int ROC_TARGET_BLOCKS = 4096;
constexpr int ROC_FIN_THREADS = 1024;

static inline long long roc_cdiv(long long a, long long b) { return (a + b - 1) / b; }

static int roc_slices(long long n_cand, long long n_scores) {
    const long long want = roc_cdiv(ROC_TARGET_BLOCKS, roc_cdiv(n_cand, ROC_THREADS));
    const long long tiles = roc_cdiv(n_scores, ROC_TILE);
    return (int)(want < tiles ? want : tiles);
}

// elements between the 16-byte-aligned address at or below p and p itself (0 .. 3)
static inline int roc_lead(const float* p) { return (int)(((uintptr_t)p >> 2) & 3); }

// Quad t of tile `tile` of the array p[0 .. n) (lead = roc_lead(p)), NaN where the quad leaves the array.
__device__ __forceinline__ f32x4 roc_load_quad(const float* __restrict__ p, int n, int lead, int tile, int t) {
    const long long e0 = (long long)tile * ROC_TILE + 4 * t - lead;    // index in p of the quad's first element
    const float nan = __int_as_float(0x7fc00000);
    f32x4 q = {nan, nan, nan, nan};
    if (e0 >= 0 && e0 + 4 <= n) {
        q = ld4(p + e0);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (e0 + k >= 0 && e0 + k < n) q[k] = p[e0 + k];
    }
    return q;
}

// cand == nullptr: the candidates are the scores themselves, [pos; neg]
__global__ __launch_bounds__(ROC_THREADS) void roc_counts_kernel(const float* __restrict__ cand, int n_cand,
                                                                 const float* __restrict__ pos, int n_pos, int lead_pos,
                                                                 const float* __restrict__ neg, int n_neg, int lead_neg,
                                                                 unsigned int* __restrict__ counts) {
    __shared__ f32x4 tile[ROC_TILE / 4];
    const int t = threadIdx.x;
    const long long ci = (long long)blockIdx.x * ROC_THREADS + t;
    float c = __int_as_float(0x7fc00000);      // a thread past the last candidate counts nothing
    if (ci < n_cand) c = cand ? cand[ci] : (ci < n_pos ? pos[ci] : neg[ci - n_pos]);

    const int tiles_pos = (int)(((long long)lead_pos + n_pos + ROC_TILE - 1) / ROC_TILE);
    const int tiles_neg = (int)(((long long)lead_neg + n_neg + ROC_TILE - 1) / ROC_TILE);
    const int tiles = tiles_pos + tiles_neg;
    const int per_slice = (tiles + (int)gridDim.y - 1) / (int)gridDim.y;
    const int t0 = (int)blockIdx.y * per_slice;
    const int t1 = t0 + per_slice < tiles ? t0 + per_slice : tiles;

    unsigned int ge = 0, lt = 0, eq = 0;
    for (int ti = t0; ti < t1; ++ti) {         // block-uniform bounds: every thread reaches both barriers
        const bool is_pos = ti < tiles_pos;
        const int tl = is_pos ? ti : ti - tiles_pos;
        const int n = is_pos ? n_pos : n_neg;
        const int lead = is_pos ? lead_pos : lead_neg;
        long long len = (long long)lead + n - (long long)tl * ROC_TILE;     // elements of this tile up to the array's end
        const int quads = (int)((len < ROC_TILE ? len : ROC_TILE) + 3) >> 2;
        __syncthreads();                        // the previous tile has been read
        if (t < quads) tile[t] = roc_load_quad(is_pos ? pos : neg, n, lead, tl, t);
        __syncthreads();
        if (is_pos) {
#pragma unroll 4
            for (int q = 0; q < quads; ++q) {
                const f32x4 s = tile[q];
                ge += (s[0] >= c) + (s[1] >= c) + (s[2] >= c) + (s[3] >= c);
            }
        } else {
#pragma unroll 4
            for (int q = 0; q < quads; ++q) {
                const f32x4 s = tile[q];
                lt += (s[0] < c) + (s[1] < c) + (s[2] < c) + (s[3] < c);
                eq += (s[0] == c) + (s[1] == c) + (s[2] == c) + (s[3] == c);
            }
        }
    }
    if (ci < n_cand) {
        atomicAdd(counts + ci, ge);
        atomicAdd(counts + (long long)n_cand + ci, lt);
        atomicAdd(counts + 2ll * n_cand + ci, eq);
    }
}

// ---------------------------------------------------------------- finish: counts of the candidates [pos; neg] -> the 8-word record
struct RocBest {
    unsigned long long key;
    unsigned int val;      // the score as an unsigned int of the same order, -0 taken as +0
    unsigned int idx;
};

__device__ __forceinline__ unsigned int roc_ordered(float v) {
    unsigned int u = __float_as_uint(v == 0.f ? 0.f : v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ bool roc_better(const RocBest& a, const RocBest& b) {      // a strictly before b
    if (a.key != b.key) return a.key > b.key;
    if (a.val != b.val) return a.val > b.val;
    return a.idx < b.idx;
}

__global__ __launch_bounds__(ROC_FIN_THREADS) void roc_finish_kernel(const float* __restrict__ pos, int n_pos,
                                                                     const float* __restrict__ neg, int n_neg,
                                                                     const unsigned int* __restrict__ counts,
                                                                     long long* __restrict__ record) {
    __shared__ unsigned long long s_w0[ROC_FIN_THREADS], s_w1[ROC_FIN_THREADS], s_key[ROC_FIN_THREADS];
    __shared__ unsigned int s_val[ROC_FIN_THREADS], s_idx[ROC_FIN_THREADS], s_nan[ROC_FIN_THREADS];
    const int t = threadIdx.x;
    const int n = n_pos + n_neg;
    unsigned long long w0 = 0, w1 = 0;
    unsigned int nans = 0;
    RocBest best = {0ull, 0u, 0xffffffffu};    // behind every candidate: index n is never reached
    for (int c = t; c < n; c += ROC_FIN_THREADS) {
        const float v = c < n_pos ? pos[c] : neg[c - n_pos];
        const unsigned int p0 = counts[c], p1 = counts[(long long)n + c], p2 = counts[2ll * n + c];
        if (c < n_pos) {
            w0 += p1;
            w1 += p2;
        }
        nans += v != v;
        const RocBest cur = {(unsigned long long)p0 * (unsigned long long)n_neg + (unsigned long long)p1 * (unsigned long long)n_pos,
                             roc_ordered(v), (unsigned int)c};
        if (roc_better(cur, best)) best = cur;
    }
    s_w0[t] = w0, s_w1[t] = w1, s_nan[t] = nans;
    s_key[t] = best.key, s_val[t] = best.val, s_idx[t] = best.idx;
    __syncthreads();
    for (int h = ROC_FIN_THREADS / 2; h > 0; h >>= 1) {
        if (t < h) {
            s_w0[t] += s_w0[t + h];
            s_w1[t] += s_w1[t + h];
            s_nan[t] += s_nan[t + h];
            const RocBest a = {s_key[t], s_val[t], s_idx[t]}, b = {s_key[t + h], s_val[t + h], s_idx[t + h]};
            if (roc_better(b, a)) s_key[t] = b.key, s_val[t] = b.val, s_idx[t] = b.idx;
        }
        __syncthreads();
    }
    if (t == 0) {
        const unsigned int i = s_idx[0];       // < n: every candidate is before the initial value
        const float v = i < (unsigned int)n_pos ? pos[i] : neg[i - n_pos];
        record[0] = (long long)s_w0[0];
        record[1] = (long long)s_w1[0];
        record[2] = (long long)s_key[0];
        record[3] = (long long)i;
        record[4] = (long long)counts[i];
        record[5] = (long long)counts[(long long)n + i];
        record[6] = (long long)s_nan[0];
        record[7] = (long long)__float_as_uint(v);
    }
}

// ---------------------------------------------------------------- entry points
static int roc_check_sizes(const char* what, long long n_cand, int n_pos, int n_neg) {
    GIM_CHECK_ARG(n_cand > 0 && n_pos > 0 && n_neg > 0, what);
    GIM_CHECK_ARG(n_cand < (1ll << 31) && (long long)n_pos + n_neg < (1ll << 31), what);
    return GIM_OK;
}

static int roc_launch_counts(const char* what, const float* cand, int n_cand, const float* pos, int n_pos, const float* neg, int n_neg,
                             uint32_t* counts, hipStream_t st) {
    if (hipMemsetAsync(counts, 0, 3ull * (size_t)n_cand * sizeof(uint32_t), st) != hipSuccess) return gim_check_launch(what);
    const dim3 grid((unsigned)roc_cdiv(n_cand, ROC_THREADS), (unsigned)roc_slices(n_cand, (long long)n_pos + n_neg));
    hipLaunchKernelGGL(roc_counts_kernel, grid, dim3(ROC_THREADS), 0, st, cand, n_cand, pos, n_pos, roc_lead(pos), neg, n_neg,
                       roc_lead(neg), counts);
    return gim_check_launch(what);
}

extern "C" int gim_roc_slices(int64_t n_cand, int64_t n_scores) {
    GIM_CHECK_ARG(n_cand > 0 && n_scores > 0 && n_cand < (1ll << 31) && n_scores < (1ll << 31), "roc_slices: sizes in [1, 2^31)");
    return roc_slices(n_cand, n_scores);
}

extern "C" int gim_roc_counts(const float* cand, int n_cand, const float* pos, int n_pos, const float* neg, int n_neg, uint32_t* counts,
                              void* stream) {
    GIM_CHECK_ARG(cand && pos && neg && counts, "roc_counts: null pointer");
    if (roc_check_sizes("roc_counts: n_cand, n_pos, n_neg positive, n_cand and n_pos + n_neg below 2^31", n_cand, n_pos, n_neg))
        return GIM_E_BADARG;
    return roc_launch_counts("gim_roc_counts", cand, n_cand, pos, n_pos, neg, n_neg, counts, (hipStream_t)stream);
}

extern "C" int gim_roc_calibrate(const float* pos, int n_pos, const float* neg, int n_neg, uint32_t* counts, int64_t* record,
                                 void* stream) {
    GIM_CHECK_ARG(pos && neg && counts && record, "roc_calibrate: null pointer");
    const long long n = (long long)n_pos + n_neg;
    if (roc_check_sizes("roc_calibrate: n_pos, n_neg positive, n_pos + n_neg below 2^31", n, n_pos, n_neg)) return GIM_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const int rc = roc_launch_counts("gim_roc_calibrate", nullptr, (int)n, pos, n_pos, neg, n_neg, counts, st);
    if (rc != GIM_OK) return rc;
    hipLaunchKernelGGL(roc_finish_kernel, dim3(1), dim3(ROC_FIN_THREADS), 0, st, pos, n_pos, neg, n_neg, counts, (long long*)record);
    return gim_check_launch("gim_roc_calibrate");
}
