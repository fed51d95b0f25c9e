// Ingest: native-size uint8 images -> the S x S uint8 image bank, reproducing PIL's Image.resize(.., BILINEAR) and convert('L')
// bit for bit (data_handling/img_datasets.py:284-303 load_image -> process_pil_image).  PIL's resampler is two separable passes
// over uint8 data - horizontal first, its result rounded to uint8, then vertical - with per-output-pixel tap windows and 22-bit
// fixed-point weights; the tables (bounds + coefficients per axis) come from the host (ingest.resample_table), the device side is
// integer only:      out = min((2^21 + sum_t src[min + t] * k[t]) >> 22, 255)      (weights >= 0: the lower clamp never acts)
//
// One workgroup = one image x one band of output rows:
//   1. the source rows the band needs are one contiguous byte range of the image; it is staged into LDS in chunks of whole rows
//      with 16-byte loads (scalar head / tail around the aligned body),
//   2. every staged row is resampled horizontally (grayscale conversion applied to the taps as they are read) into the band's LDS
//      tile [rows][out_w][C_out] uint8 (one pixel's channels, or four one-channel taps, per pair of aligned LDS words),
//   3. the vertical pass runs out of the tile, 4 output bytes per lane where the output row length allows.
// An axis without tables is copied.  Every table entry is clamped to the image and to the tile before it is used as an index, so
// that a wrong table gives wrong pixels, never an access outside src, dst or LDS.
#include "common.h"

namespace {

constexpr int INGEST_THREADS = 256;
constexpr int INGEST_RAW_BYTES = 16384;                         // staging buffer for source rows (whole rows per chunk)
constexpr int INGEST_LDS_MAX = 65536;                           // dynamic LDS of one workgroup without opt-in
constexpr int INGEST_RAW_SLACK = 32;                            // raw keeps the source's 16-byte phase (<= 15) + lds_load4's over-read (<= 7)
constexpr int INGEST_TILE_MAX = INGEST_LDS_MAX - INGEST_RAW_BYTES - INGEST_RAW_SLACK;   // 49120
constexpr int INGEST_TILE_PREF = 24576;                         // preferred tile: 40 KiB per workgroup, 4 workgroups per CU
constexpr long long INGEST_MAX_GRID = 65536;                    // workgroups per launch; (image, band) items beyond it are looped over
constexpr int PREC_BITS = 22;                                   // PIL: PRECISION_BITS = 32 - 8 - 2

struct IngestArgs {
    const uint8_t* src;
    uint8_t* dst;
    const int32_t *x_bounds, *x_coef, *y_bounds, *y_coef;
    long long n_items;   // n_img * n_bands
    int H, W, out_h, out_w, x_ksize, y_ksize;
    int band_h, n_bands, tile_rows, raw_rows;
};

// PIL's clip8.  The weights of the triangle filter are >= 0, so the accumulator (< 2^31: 2^21 + 255 * (2^22 + ksize)) never goes
// negative and only the upper clamp can act; the shift is therefore done unsigned.  That is also what keeps the packed store of the
// vertical pass right: two SIGNED shift-and-clamp results merged into one word compile to v_ashr_pk_u8_i32, whose upper 16 result
// bits were seen to keep the register's previous contents on the MI355X (they ended up ORed into bytes 2 and 3 of the word).
__device__ __forceinline__ uint32_t clip8(uint32_t acc) {
    const uint32_t v = acc >> PREC_BITS;
    return v > 255u ? 255u : v;
}
constexpr uint32_t ACC0 = 1u << (PREC_BITS - 1);

// value (<= 255) * weight (<= 2^22) on the full-rate 24-bit multiplier
__device__ __forceinline__ uint32_t mul8x22(uint32_t v, int k) { return __umul24(v, (uint32_t)k); }

// The 4 bytes at ANY byte offset of a 4-byte aligned LDS array: two aligned words and a byte alignment, instead of 4 byte reads
// (which also collide on the banks: neighbouring lanes read windows a few bytes apart).  Reads up to 7 bytes past `off`.
__device__ __forceinline__ uint32_t lds_load4(const uint32_t* words, int off) {
    const uint32_t* w = words + (off >> 2);
    return __builtin_amdgcn_alignbyte(w[1], w[0], (uint32_t)(off & 3));
}

// ITU-R 601-2 luma as PIL's convert('L') rounds it; rgb = R | G << 8 | B << 16 (| anything << 24)
__device__ __forceinline__ uint32_t luma(uint32_t rgb) {
    return ((rgb & 255u) * 19595u + ((rgb >> 8) & 255u) * 38470u + ((rgb >> 16) & 255u) * 7471u + 0x8000u) >> 16;
}

// [min, min + cnt) of output index i, clamped to [0, size) and to ksize taps; no table: the identity.
__device__ __forceinline__ void tap_window(const int32_t* bounds, int i, int size, int ksize, int& mn, int& cnt) {
    if (!bounds) {
        mn = i;
        cnt = 1;
        return;
    }
    mn = bounds[2 * i];
    cnt = bounds[2 * i + 1];
    mn = mn < 0 ? 0 : (mn > size ? size : mn);
    cnt = cnt < 0 ? 0 : cnt;
    cnt = cnt > ksize ? ksize : cnt;
    cnt = cnt > size - mn ? size - mn : cnt;
}

template <int CIN, bool GRAY>
__global__ __launch_bounds__(INGEST_THREADS) void resize_bilinear_u8_kernel(const IngestArgs a) {
    constexpr int COUT = GRAY ? 1 : CIN;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    uint8_t* const tile = lds;                                            // [tile_rows][out_w][COUT]
    uint8_t* const raw = lds + (((long long)a.tile_rows * a.out_w * COUT + 15) & ~15LL);   // INGEST_RAW_BYTES + INGEST_RAW_SLACK
    const uint32_t* const raw32 = (const uint32_t*)raw;
    const int tid = threadIdx.x;
    const int src_row_bytes = a.W * CIN, out_row_bytes = a.out_w * COUT;

    for (long long item = blockIdx.x; item < a.n_items; item += gridDim.x) {
        const long long img = item / a.n_bands;
        const int y0 = (int)(item - img * a.n_bands) * a.band_h;
        const int y1 = min(y0 + a.band_h, a.out_h);
        // source rows [r0, r0 + rows) of this band (the windows move monotonically with y)
        int r0, cnt, rl, rows;
        tap_window(a.y_bounds, y0, a.H, a.y_ksize, r0, cnt);
        tap_window(a.y_bounds, y1 - 1, a.H, a.y_ksize, rl, cnt);
        rows = min(max(rl + cnt - r0, 0), a.tile_rows);

        // ---- passes 1 + 2: stage whole source rows, resample them horizontally into the tile
        for (int done = 0; done < rows; done += a.raw_rows) {
            const int cr = min(a.raw_rows, rows - done);
            const uint8_t* g = a.src + ((img * a.H + r0 + done) * (long long)src_row_bytes);
            const int nbytes = cr * src_row_bytes;
            const int phase = (int)((uintptr_t)g & 15);
            uint8_t* const rawp = raw + phase;                            // same 16-byte phase as the source
            const int head = min(nbytes, (16 - phase) & 15);
            const int nvec = (nbytes - head) >> 4;
            const int tail0 = head + (nvec << 4);
            for (int i = tid; i < nvec; i += INGEST_THREADS)
                *(uint4*)(rawp + head + (i << 4)) = *(const uint4*)(g + head + (i << 4));
            if (tid < head) rawp[tid] = g[tid];
            if (tid < nbytes - tail0) rawp[tail0 + tid] = g[tail0 + tid];
            __syncthreads();
            for (int i = tid; i < cr * a.out_w; i += INGEST_THREADS) {
                const int r = i / a.out_w, xx = i - r * a.out_w;
                const int row = phase + r * src_row_bytes;                // byte offset of the staged row in raw
                uint8_t* o = tile + ((done + r) * a.out_w + xx) * COUT;
                int xmin, xcnt;
                tap_window(a.x_bounds, xx, a.W, a.x_ksize, xmin, xcnt);
                const int32_t* k = a.x_coef + (long long)xx * a.x_ksize;  // not read without tables
                if (CIN == 1) {
                    uint32_t acc = ACC0;
                    if (!a.x_bounds) {
                        acc = (lds_load4(raw32, row + xmin) & 255u) << PREC_BITS;
                    } else {
                        for (int t = 0; t < xcnt; t += 4) {               // the taps of one output pixel are consecutive bytes
                            const uint32_t v = lds_load4(raw32, row + xmin + t);
                            acc += mul8x22(v & 255u, k[t]);
                            if (t + 1 < xcnt) acc += mul8x22((v >> 8) & 255u, k[t + 1]);
                            if (t + 2 < xcnt) acc += mul8x22((v >> 16) & 255u, k[t + 2]);
                            if (t + 3 < xcnt) acc += mul8x22(v >> 24, k[t + 3]);
                        }
                    }
                    o[0] = (uint8_t)clip8(acc);
                } else if (GRAY) {
                    uint32_t acc = ACC0;
                    if (!a.x_bounds) {
                        acc = luma(lds_load4(raw32, row + 3 * xmin)) << PREC_BITS;
                    } else {
                        for (int t = 0; t < xcnt; ++t) acc += mul8x22(luma(lds_load4(raw32, row + 3 * (xmin + t))), k[t]);
                    }
                    o[0] = (uint8_t)clip8(acc);
                } else {
                    uint32_t a0 = ACC0, a1 = ACC0, a2 = ACC0;
                    if (!a.x_bounds) {
                        const uint32_t v = lds_load4(raw32, row + 3 * xmin);
                        a0 = (v & 255u) << PREC_BITS;
                        a1 = ((v >> 8) & 255u) << PREC_BITS;
                        a2 = ((v >> 16) & 255u) << PREC_BITS;
                    } else {
                        for (int t = 0; t < xcnt; ++t) {
                            const uint32_t v = lds_load4(raw32, row + 3 * (xmin + t));
                            const int kv = k[t];
                            a0 += mul8x22(v & 255u, kv);
                            a1 += mul8x22((v >> 8) & 255u, kv);
                            a2 += mul8x22((v >> 16) & 255u, kv);
                        }
                    }
                    o[0] = (uint8_t)clip8(a0);
                    o[1] = (uint8_t)clip8(a1);
                    o[2] = (uint8_t)clip8(a2);
                }
            }
            __syncthreads();
        }

        // ---- pass 3: vertical, tile -> dst (the band's output rows are one contiguous byte range)
        uint8_t* const d = a.dst + ((img * a.out_h + y0) * (long long)out_row_bytes);
        const int n_out = (y1 - y0) * out_row_bytes;
        if ((out_row_bytes & 3) == 0 && ((uintptr_t)a.dst & 3) == 0) {
            for (int i = tid; i < (n_out >> 2); i += INGEST_THREADS) {
                const int o = i << 2;
                const int yb = o / out_row_bytes, j = o - yb * out_row_bytes;
                int ymin, ycnt;
                tap_window(a.y_bounds, y0 + yb, a.H, a.y_ksize, ymin, ycnt);
                const int lo = max(ymin, r0), hi = min(ymin + ycnt, r0 + rows);
                uint32_t packed;
                if (!a.y_bounds) {
                    packed = lo < hi ? *(const uint32_t*)(tile + (lo - r0) * out_row_bytes + j) : 0u;
                } else {
                    const int32_t* k = a.y_coef + (long long)(y0 + yb) * a.y_ksize;
                    uint32_t a0 = ACC0, a1 = ACC0, a2 = ACC0, a3 = ACC0;
                    for (int r = lo; r < hi; ++r) {
                        const uint32_t v = *(const uint32_t*)(tile + (r - r0) * out_row_bytes + j);
                        const int kv = k[r - ymin];
                        a0 += mul8x22(v & 255u, kv);
                        a1 += mul8x22((v >> 8) & 255u, kv);
                        a2 += mul8x22((v >> 16) & 255u, kv);
                        a3 += mul8x22(v >> 24, kv);
                    }
                    packed = clip8(a0) | (clip8(a1) << 8) | (clip8(a2) << 16) | (clip8(a3) << 24);
                }
                *(uint32_t*)(d + o) = packed;
            }
        } else {
            for (int o = tid; o < n_out; o += INGEST_THREADS) {
                const int yb = o / out_row_bytes, j = o - yb * out_row_bytes;
                int ymin, ycnt;
                tap_window(a.y_bounds, y0 + yb, a.H, a.y_ksize, ymin, ycnt);
                const int lo = max(ymin, r0), hi = min(ymin + ycnt, r0 + rows);
                uint32_t v;
                if (!a.y_bounds) {
                    v = lo < hi ? tile[(lo - r0) * out_row_bytes + j] : 0u;
                } else {
                    const int32_t* k = a.y_coef + (long long)(y0 + yb) * a.y_ksize;
                    uint32_t acc = ACC0;
                    for (int r = lo; r < hi; ++r) acc += mul8x22(tile[(r - r0) * out_row_bytes + j], k[r - ymin]);
                    v = clip8(acc);
                }
                d[o] = (uint8_t)v;
            }
        }
        // the next item's first tile write comes after a barrier that every thread reaches only after this pass
    }
}

// Upper bound of the source rows that `band_h` consecutive output rows read: window ends and starts differ by at most
// (band_h - 1) * H / out_h + 2 * support + 1 <= ceil((band_h - 1) * H / out_h) + ksize.
long long band_src_rows(int band_h, int H, int out_h, int y_ksize) {
    if (y_ksize == 0) return band_h;
    const long long r = ((long long)(band_h - 1) * H + out_h - 1) / out_h + y_ksize;
    return r < H ? r : H;
}

}  // namespace

extern "C" int gim_resize_bilinear_u8(const uint8_t* src, int64_t n_img, int H, int W, int C_in, int to_gray, uint8_t* dst, int out_h,
                                      int out_w, const int32_t* x_bounds, const int32_t* x_coef, int x_ksize, const int32_t* y_bounds,
                                      const int32_t* y_coef, int y_ksize, void* stream) {
    GIM_CHECK_ARG(src && dst && n_img > 0 && H > 0 && W > 0 && out_h > 0 && out_w > 0, "resize_bilinear_u8: bad args");
    GIM_CHECK_ARG(C_in == 1 || C_in == 3, "resize_bilinear_u8: C_in must be 1 or 3");
    GIM_CHECK_ARG(!to_gray || C_in == 3, "resize_bilinear_u8: to_gray needs C_in == 3");
    GIM_CHECK_ARG(x_ksize >= 0 && y_ksize >= 0, "resize_bilinear_u8: negative tap count");
    GIM_CHECK_ARG((x_bounds != nullptr) == (x_ksize > 0) && (x_coef != nullptr) == (x_ksize > 0),
                  "resize_bilinear_u8: x_bounds, x_coef and x_ksize go together (NULL, NULL, 0 = copy)");
    GIM_CHECK_ARG((y_bounds != nullptr) == (y_ksize > 0) && (y_coef != nullptr) == (y_ksize > 0),
                  "resize_bilinear_u8: y_bounds, y_coef and y_ksize go together (NULL, NULL, 0 = copy)");
    GIM_CHECK_ARG(x_ksize > 0 || W == out_w, "resize_bilinear_u8: no x tables although W != out_w");
    GIM_CHECK_ARG(y_ksize > 0 || H == out_h, "resize_bilinear_u8: no y tables although H != out_h");
    const int C_out = to_gray ? 1 : C_in;
    GIM_CHECK_ARG((long long)W * C_in <= INGEST_RAW_BYTES, "resize_bilinear_u8: a source row (W * C_in) is longer than the 16384-byte staging buffer");
    const long long out_row_bytes = (long long)out_w * C_out;
    GIM_CHECK_ARG(band_src_rows(1, H, out_h, y_ksize) * out_row_bytes <= INGEST_TILE_MAX,
                  "resize_bilinear_u8: the LDS tile of a one-row band (min(y_ksize, H) * out_w * C_out bytes) exceeds 49120 bytes: shrink factor too large");
    // band height: the tallest band whose tile stays within the preferred size; a single row may use the whole budget
    int band_h = 1;
    while (band_h < out_h && band_src_rows(band_h + 1, H, out_h, y_ksize) * out_row_bytes <= INGEST_TILE_PREF) ++band_h;
    IngestArgs a;
    a.src = src;
    a.dst = dst;
    a.x_bounds = x_bounds;
    a.x_coef = x_coef;
    a.y_bounds = y_bounds;
    a.y_coef = y_coef;
    a.H = H;
    a.W = W;
    a.out_h = out_h;
    a.out_w = out_w;
    a.x_ksize = x_ksize;
    a.y_ksize = y_ksize;
    a.band_h = band_h;
    a.n_bands = (out_h + band_h - 1) / band_h;
    a.n_items = (long long)n_img * a.n_bands;
    a.tile_rows = (int)band_src_rows(band_h, H, out_h, y_ksize);
    a.raw_rows = INGEST_RAW_BYTES / (W * C_in);
    const size_t lds = (size_t)((a.tile_rows * out_row_bytes + 15) & ~15LL) + INGEST_RAW_BYTES + INGEST_RAW_SLACK;
    const dim3 grid((unsigned)(a.n_items < INGEST_MAX_GRID ? a.n_items : INGEST_MAX_GRID)), block(INGEST_THREADS);
    hipStream_t st = (hipStream_t)stream;
    if (to_gray)
        hipLaunchKernelGGL((resize_bilinear_u8_kernel<3, true>), grid, block, lds, st, a);
    else if (C_in == 3)
        hipLaunchKernelGGL((resize_bilinear_u8_kernel<3, false>), grid, block, lds, st, a);
    else
        hipLaunchKernelGGL((resize_bilinear_u8_kernel<1, false>), grid, block, lds, st, a);
    return gim_check_launch("gim_resize_bilinear_u8");
}
