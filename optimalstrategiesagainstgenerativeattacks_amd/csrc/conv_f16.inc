// fp16-operand variants of the implicit-GEMM convolution kernels (included by conv_igemm.hip after its shared definitions).
//
// BASELINE config 5 names "fp16 MFMA" (128x128x3, m=5 n=20 k=20).  The reference has no 16-bit path; this is the engine's opt-in
// one (gim_conv_shape.prec = 1, ops.set_matrix_path("fp16")): v_mfma_f32_32x32x16_f16, fp32 accumulate, fp32 master weights and
// fp32 activations in HBM.  Operands are rounded to fp16 (round to nearest even, v_cvt_pk_f16_f32) when they are staged into LDS,
// AFTER the fused LeakyReLU; everything behind the accumulators (1/sigma, bias, residual, masks, atomics) is the fp32 epilogue of
// the fp32 kernels.  16x the matrix rate of the fp32 MFMA means these kernels are bound by operand traffic, not by the matrix
// pipe: a 128 x 128 tile moves 32 KB of fp32 operands per 32-deep K step and spends 256 matrix cycles on it.
//
//   conv_igemm_f16_kernel : forward-style launches (BMODE 0: k-contiguous weight rows) of every geometry of struct Geo - forward
//                           (plain, pool-folded S2, sub-pixel PC) and dgrad on TRANSPOSED weights (gim_conv2d_dgrad_t: the host
//                           routes every fp16 dgrad there).  Fast path only: Ca % 32 == 0, 16-byte aligned operands.
//   conv_wgrad_f16_kernel : weight gradient, 128 x 128 tile, 32 pixels per K step; both operands are contracted over their SLOW
//                           (pixel) index, so their LDS images [pixel][channel] are read through ds_read_b64_tr_b16 (the
//                           transposing LDS read of gfx950) with the XOR swizzle that keeps row and transposed reads conflict-free.
typedef _Float16 h8_t __attribute__((ext_vector_type(8)));
typedef _Float16 h4_t __attribute__((ext_vector_type(4)));
typedef _Float16 h2_t __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

// fp32 -> fp16, round to nearest even, SATURATING at +-65504: an activation or gradient beyond the fp16 range becomes the largest
// finite value instead of an infinity (inf - inf, 0 * inf = NaN two layers later).  SAT = false for weights (spectrally normalised
// elsewhere, |w| << 65504: no clamp instructions spent on them).  The host keeps gradients inside the range from the other side with
// a loss scale (ops.loss_scale): fp16 is precise down to 6e-5 only, gradients of a mean loss sit at 1e-3 ... 1e-7.
// The three kernels below carry the clamp of their PIXEL-side operands as a compile-time flag (kernel parameter SAT, default true =
// gim_conv_shape.prec 1).  SAT = false (prec 2) is the plain IEEE conversion: |value| >= 65520 becomes +-inf and travels through the
// fp32 accumulators into the output as it would in fp32 arithmetic - what a dynamic loss scaler detects in the gradient bucket
// (gim_adam_step_scaled).  Same tiles, same LDS images, same loops: the two instantiations differ in the v_med3_f32 per element only.
template <bool SAT>
__device__ __forceinline__ f32x4 sat16(f32x4 v) {
    if constexpr (SAT) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = __builtin_amdgcn_fmed3f(v[e], -65504.f, 65504.f);
    }
    return v;
}
template <bool SAT>
__device__ __forceinline__ h8_t cvt8_f16(f32x4 lo, f32x4 hi) {
    lo = sat16<SAT>(lo); hi = sat16<SAT>(hi);
    const h2_t a = __builtin_convertvector(f32x2{lo[0], lo[1]}, h2_t), b = __builtin_convertvector(f32x2{lo[2], lo[3]}, h2_t);
    const h2_t c = __builtin_convertvector(f32x2{hi[0], hi[1]}, h2_t), d = __builtin_convertvector(f32x2{hi[2], hi[3]}, h2_t);
    return h8_t{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}
template <bool SAT>
__device__ __forceinline__ h4_t cvt4_f16(f32x4 v) {
    v = sat16<SAT>(v);
    const h2_t a = __builtin_convertvector(f32x2{v[0], v[1]}, h2_t), b = __builtin_convertvector(f32x2{v[2], v[3]}, h2_t);
    return h4_t{a[0], a[1], b[0], b[1]};
}

// K step: 32 channels of one tap.  LDS rows of 32 halves (64 B) padded to 80 B: byte for byte the image of the fp32 kernel's
// 16-float rows, so the same conflict-free ds_write_b128 / ds_read_b128 pattern; a 16-byte fragment is 8 k values = one MFMA operand.
template <int BM, int BN, int TM, int TN, bool SAT = true>
__global__ __launch_bounds__(256, 2) void conv_igemm_f16_kernel(const ConvP p) {
    constexpr int KB = 32, LDH = 40;              // halves per padded LDS row
    constexpr int WAVES_N = BN / (32 * TN), WAVES_M = BM / (32 * TM);
    static_assert(WAVES_M * WAVES_N == 4, "4 waves per workgroup");
    constexpr int A_ROWS = BM / 64, B_ROWS = BN / 64;   // 64 tile rows per pass: 4 threads x 8 k values per row
    constexpr int A_SZ = BM * LDH, B_SZ = BN * LDH;
    __shared__ __attribute__((aligned(16))) _Float16 lds[2 * A_SZ + 2 * B_SZ];
    _Float16* As = lds;
    _Float16* Bs = lds + 2 * A_SZ;

    Geo g = p.g;
    int kslice = blockIdx.z;
    if (g.pc) {
        geo_select_class(g, blockIdx.z & 3);
        kslice = blockIdx.z >> 2;
    }
    const int t = threadIdx.x;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    const int arow = t >> 2, aq = (t & 3) * 8;
    const int He = g.Hin << g.ups, We = g.Win << g.ups;
    const int KF2 = g.KF * g.KFw;
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, p.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, 0xFFFFFFFFu, 0x00020000);
    int a_oy[A_ROWS], a_ox[A_ROWS];
    unsigned a_base[A_ROWS], a_cur[A_ROWS], b_voff[B_ROWS];
#pragma unroll
    for (int i = 0; i < A_ROWS; ++i) {
        const int m = min(m0 + arow + 64 * i, p.M - 1);
        const int n = m >> (g.logH + g.logW);
        a_oy[i] = ((m >> g.logW) & (g.H - 1)) * g.s_in + g.off_y;
        a_ox[i] = (m & (g.W - 1)) * g.s_in_x + g.off_x;
        a_base[i] = (unsigned)((n * g.Hin * g.Win * p.Ca + aq) * 4);
        a_cur[i] = BUF_OOB;
    }
#pragma unroll
    for (int i = 0; i < B_ROWS; ++i) {
        const int row = min(n0 + arow + 64 * i, p.Cb - 1);
        b_voff[i] = (unsigned)((row * KF2 * p.Cin_w + aq) * 4);
    }
    auto set_tap = [&](int ta, int tb) {
#pragma unroll
        for (int i = 0; i < A_ROWS; ++i) {
            const int iy = a_oy[i] + ta, ix = a_ox[i] + tb;
            const bool v = (unsigned)iy < (unsigned)He && (unsigned)ix < (unsigned)We;
            const int py = g.ups ? (iy >> 1) : iy, px = g.ups ? (ix >> 1) : ix;
            a_cur[i] = v ? a_base[i] + (unsigned)((py * g.Win + px) * p.Ca * 4) : BUF_OOB;
        }
    };
    f32x4 ra[A_ROWS][2], rb[B_ROWS][2];
    int k_c0 = 0, k_ta = 0, k_tb = 0;
    auto seek = [&](int k0) {
        const int tap = k0 / p.Ca;
        k_c0 = k0 - tap * p.Ca;
        k_ta = tap / g.Tw;
        k_tb = tap - k_ta * g.Tw;
        set_tap(k_ta, k_tb);
    };
    auto load_tiles = [&]() {
        const int wtap = (g.wa_base + g.wa_step * k_ta) * g.KFw + g.wb_base + g.wb_step * k_tb;
        const unsigned sa = (unsigned)(k_c0 * 4);
#pragma unroll
        for (int i = 0; i < A_ROWS; ++i) {
            ra[i][0] = buf_load4(rx, a_cur[i], sa);
            ra[i][1] = buf_load4(rx, a_cur[i], sa + 16u);   // (an out-of-range lane offset stays out of range: the SGPR offset is not part of the bounds test)
        }
        const unsigned sb = (unsigned)((wtap * p.Cin_w + k_c0) * 4);
#pragma unroll
        for (int i = 0; i < B_ROWS; ++i) {
            rb[i][0] = buf_load4(rw, b_voff[i], sb);
            rb[i][1] = buf_load4(rw, b_voff[i], sb + 16u);
        }
        k_c0 += KB;
        if (k_c0 == p.Ca) {
            k_c0 = 0;
            if (++k_tb == g.Tw) { k_tb = 0; ++k_ta; }
            set_tap(k_ta, k_tb);
        }
    };
    const bool has_act = p.pre_slope != 1.0f;
    auto store_tiles = [&](int buf) {
#pragma unroll
        for (int i = 0; i < A_ROWS; ++i) {
            if (has_act) {
#pragma unroll
                for (int q = 0; q < 2; ++q)
#pragma unroll
                    for (int e = 0; e < 4; ++e) ra[i][q][e] = __builtin_amdgcn_fmed3f(ra[i][q][e], ra[i][q][e] * p.pre_slope, p.pos_inf);
            }
            *reinterpret_cast<h8_t*>(&As[buf * A_SZ + (arow + 64 * i) * LDH + aq]) = cvt8_f16<SAT>(ra[i][0], ra[i][1]);
        }
#pragma unroll
        for (int i = 0; i < B_ROWS; ++i)
            *reinterpret_cast<h8_t*>(&Bs[buf * B_SZ + (arow + 64 * i) * LDH + aq]) = cvt8_f16<false>(rb[i][0], rb[i][1]);
    };
    const int lane = t & 63, r = lane & 31, h = lane >> 5, wv = t >> 6;
    const int wm0 = (wv / WAVES_N) * 32 * TM, wn0 = (wv % WAVES_N) * 32 * TN;
    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    const int nk_all = p.Ktot / KB;
    const int ks0 = kslice * p.kper;
    const int nk = min(nk_all, ks0 + p.kper);
    seek(ks0 * KB);
    load_tiles();
    store_tiles(0);
    __syncthreads();
    auto kstep = [&](int ks, auto BUFC, auto MAINC) {
        constexpr int buf = decltype(BUFC)::value;
        constexpr bool MAIN = decltype(MAINC)::value;
        if (MAIN || ks + 1 < nk) load_tiles();
        __builtin_amdgcn_sched_barrier(0);
        const _Float16* Ab = As + buf * A_SZ;
        const _Float16* Bb = Bs + buf * B_SZ;
        h8_t a[2][TM], b[2][TN];
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
            for (int i = 0; i < TM; ++i) a[kk][i] = *reinterpret_cast<const h8_t*>(&Ab[(wm0 + 32 * i + r) * LDH + 16 * kk + 8 * h]);
#pragma unroll
            for (int j = 0; j < TN; ++j) b[kk][j] = *reinterpret_cast<const h8_t*>(&Bb[(wn0 + 32 * j + r) * LDH + 16 * kk + 8 * h]);
        }
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[kk][i], b[kk][j], acc[i][j], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        if (MAIN || ks + 1 < nk) store_tiles(buf ^ 1);
        __syncthreads();
    };
    int ks = ks0;
    for (; ks + 2 < nk; ks += 2) {
        kstep(ks, std::integral_constant<int, 0>(), std::true_type());
        kstep(ks + 1, std::integral_constant<int, 1>(), std::true_type());
    }
    for (; ks < nk; ks += 2) {
        kstep(ks, std::integral_constant<int, 0>(), std::false_type());
        if (ks + 1 < nk) kstep(ks + 1, std::integral_constant<int, 1>(), std::false_type());
    }

    // ---- epilogue: the fp32 kernels' (epi_fill, epi_dispatch, epi_block) ----
    EpiCtx ec;
    const bool first = kslice == 0;
    bool has_res, has_mask;
    epi_fill<false, false>(ec, p, g, first, has_res, has_mask);
    auto run = [&](auto MODEC) {
        constexpr int MODE = decltype(MODEC)::value;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int co = n0 + wn0 + 32 * j + r;
                const bool cok = co < p.Cb;
                const float bv = (p.bias && first && cok) ? p.bias[co] : 0.f;
                float a_[16];
#pragma unroll
                for (int e = 0; e < 16; ++e) a_[e] = acc[i][j][e];
                epi_block<16, MODE>(ec, a_, m0 + wm0 + 32 * i + 4 * h, co, cok, bv);
            }
    };
    epi_dispatch<0, 0>(p, has_res, has_mask, run);
}

// -------------------------------------------------------------------------------------------------
// Patch-resident fp16 form for plain 3x3 convolutions (conv_igemm_patch_kernel's loop, BMODE 0 only: forward, and dgrad on transposed
// weights).  The fp16 kernels are bound by operand traffic; the tap-major loop above re-reads every activation row once per tap
// (9x for a 3x3 layer, from L2), this one loads the (rows + 2) x (columns + 2) input patch of a tile once per 32-channel chunk, rounds it
// once and serves all nine taps from LDS.  Byte for byte the LDS images of the fp32 patch kernel (80-byte rows = 32 halves + pad).
// Host guarantees as for conv_igemm_patch_kernel, with Ca % 32 == 0 and split-K in whole 32-channel chunks.
// -------------------------------------------------------------------------------------------------
template <int BM, int BN, int TM, int TN, bool SAT = true>
__global__ __launch_bounds__(256, 2) void conv_igemm_patch_f16_kernel(const ConvP p) {
    constexpr int KB = 32, LDH = 40;
    constexpr int WAVES_N = BN / (32 * TN), WAVES_M = BM / (32 * TM);
    static_assert(WAVES_M * WAVES_N == 4, "4 waves per workgroup");
    constexpr int P_PER = BM == 64 ? 4 : 5;          // patch slots (pixel, 8-channel group) per thread
    constexpr int B_ROWS = BN / 64;
    constexpr int B_SZ = BN * LDH;                   // halves
    extern __shared__ __attribute__((aligned(16))) _Float16 patch16_lds[];
    const Geo& g = p.g;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int kslice = blockIdx.z;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    const int Wt = min(g.W, BM), logWt = 31 - __builtin_clz(Wt);
    const int PW = Wt + 2, PP = (BM / Wt + 2) * PW;
    const int P_SZ = (PP * LDH + 7) & ~7;            // halves, 16-byte multiple
    _Float16* Ps = patch16_lds;
    _Float16* Bs = patch16_lds + 2 * P_SZ;
    const int n_img = m0 >> (g.logH + g.logW);
    const int oy0 = ((m0 >> g.logW) & (g.H - 1)) + g.off_y, ox0 = (m0 & (g.W - 1)) + g.off_x;
    const int KF2 = g.KF * g.KFw;
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, p.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, 0xFFFFFFFFu, 0x00020000);
    unsigned p_voff[P_PER];
    int p_lds[P_PER];
#pragma unroll
    for (int i = 0; i < P_PER; ++i) {
        const int q = t + 256 * i, pp = q >> 2, grp = q & 3;
        const int pr = pp / PW, pc = pp - pr * PW;
        const int iy = oy0 + pr, ix = ox0 + pc;
        const bool v = pp < PP && (unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.W;
        p_voff[i] = v ? (unsigned)((((n_img * g.Hin + iy) * g.Win + ix) * p.Ca + grp * 8) * 4) : BUF_OOB;
        p_lds[i] = pp < PP ? pp * LDH + grp * 8 : -1;
    }
    unsigned b_voff[B_ROWS];
    const int brow = t >> 2, bq = (t & 3) * 8;
#pragma unroll
    for (int i = 0; i < B_ROWS; ++i) b_voff[i] = (unsigned)((min(n0 + brow + 64 * i, p.Cb - 1) * KF2 * p.Cin_w + bq) * 4);
    const bool has_act = p.pre_slope != 1.0f;
    f32x4 rp[P_PER][2], rb[B_ROWS][2];
    auto load_patch = [&](int c0) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < P_PER; ++i) {
            rp[i][0] = buf_load4(rx, p_voff[i], (unsigned)(c0 * 4));
            rp[i][1] = buf_load4(rx, p_voff[i], (unsigned)(c0 * 4) + 16u);
        }
    };
    int p_wr = 0;
    auto store_patch = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < P_PER; ++i) {
            if (has_act) {
#pragma unroll
                for (int q = 0; q < 2; ++q)
#pragma unroll
                    for (int e = 0; e < 4; ++e) rp[i][q][e] = __builtin_amdgcn_fmed3f(rp[i][q][e], rp[i][q][e] * p.pre_slope, p.pos_inf);
            }
            if (p_lds[i] >= 0) *reinterpret_cast<h8_t*>(&Ps[p_wr + p_lds[i]]) = cvt8_f16<SAT>(rp[i][0], rp[i][1]);
        }
        p_wr = p_wr ? 0 : P_SZ;
    };
    auto load_b = [&](int ta, int tb, int c0) __attribute__((always_inline)) {
        const int wtap = (g.wa_base + g.wa_step * ta) * g.KFw + g.wb_base + g.wb_step * tb;
        const unsigned sb = (unsigned)((wtap * p.Cin_w + c0) * 4);
#pragma unroll
        for (int i = 0; i < B_ROWS; ++i) {
            rb[i][0] = buf_load4(rw, b_voff[i], sb);
            rb[i][1] = buf_load4(rw, b_voff[i], sb + 16u);
        }
    };
    auto store_b = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < B_ROWS; ++i) *reinterpret_cast<h8_t*>(&Bs[buf * B_SZ + (brow + 64 * i) * LDH + bq]) = cvt8_f16<false>(rb[i][0], rb[i][1]);
    };
    const int r = lane & 31, h = lane >> 5;
    const int wm0 = (wv / WAVES_N) * 32 * TM, wn0 = (wv % WAVES_N) * 32 * TN;
    int a_row[3][TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int q = wm0 + 32 * i + r;
        const int base = ((q >> logWt) * PW + (q & (Wt - 1))) * LDH + 8 * h;
#pragma unroll
        for (int ta = 0; ta < 3; ++ta) a_row[ta][i] = base + ta * PW * LDH;
    }
    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    const int nchunk = p.Ca / KB;
    const int ch0 = kslice * (p.kper / 9);
    const int ch1 = min(nchunk, ch0 + p.kper / 9);
    load_patch(ch0 * KB);
    load_b(0, 0, ch0 * KB);
    store_patch();
    store_b(0);
    __syncthreads();
    auto kstep = [&](int ch, bool more_chunks, auto TAPC, auto BBC) __attribute__((always_inline)) {
        constexpr int TAP = decltype(TAPC)::value, BB = decltype(BBC)::value;
        constexpr int TA = TAP / 3, TB = TAP % 3;
        if (TAP == 0 && more_chunks) load_patch((ch + 1) * KB);
        if (TAP < 8) load_b((TAP + 1) / 3, (TAP + 1) % 3, ch * KB);
        else if (more_chunks) load_b(0, 0, (ch + 1) * KB);
        __builtin_amdgcn_sched_barrier(0);
        const _Float16* Bb = Bs + BB * B_SZ;
        h8_t a[2][TM], b[2][TN];
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
            for (int i = 0; i < TM; ++i) a[kk][i] = *reinterpret_cast<const h8_t*>(&Ps[a_row[TA][i] + TB * LDH + 16 * kk]);
#pragma unroll
            for (int j = 0; j < TN; ++j) b[kk][j] = *reinterpret_cast<const h8_t*>(&Bb[(wn0 + 32 * j + r) * LDH + 16 * kk + 8 * h]);
        }
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[kk][i], b[kk][j], acc[i][j], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        if (TAP < 8 || more_chunks) store_b(BB ^ 1);
        if (TAP == 8 && more_chunks) store_patch();
        __syncthreads();
    };
    int pbuf = 0;
    auto chunk = [&](int ch, auto B0C) __attribute__((always_inline)) {
        constexpr int B0 = decltype(B0C)::value;
        using Ba = std::integral_constant<int, B0>;
        using Bb_ = std::integral_constant<int, B0 ^ 1>;
        const bool more_chunks = ch + 1 < ch1;
        kstep(ch, more_chunks, std::integral_constant<int, 0>(), Ba());
        kstep(ch, more_chunks, std::integral_constant<int, 1>(), Bb_());
        kstep(ch, more_chunks, std::integral_constant<int, 2>(), Ba());
        kstep(ch, more_chunks, std::integral_constant<int, 3>(), Bb_());
        kstep(ch, more_chunks, std::integral_constant<int, 4>(), Ba());
        kstep(ch, more_chunks, std::integral_constant<int, 5>(), Bb_());
        kstep(ch, more_chunks, std::integral_constant<int, 6>(), Ba());
        kstep(ch, more_chunks, std::integral_constant<int, 7>(), Bb_());
        kstep(ch, more_chunks, std::integral_constant<int, 8>(), Ba());
        const int d = pbuf ? -P_SZ : P_SZ;
        pbuf ^= 1;
#pragma unroll
        for (int ta = 0; ta < 3; ++ta)
#pragma unroll
            for (int i = 0; i < TM; ++i) a_row[ta][i] += d;
    };
    int ch = ch0;
    for (; ch + 1 < ch1; ch += 2) {
        chunk(ch, std::integral_constant<int, 0>());
        chunk(ch + 1, std::integral_constant<int, 1>());
    }
    if (ch < ch1) chunk(ch, std::integral_constant<int, 0>());

    EpiCtx ec;
    const bool first = kslice == 0;
    bool has_res, has_mask;
    epi_fill<true, false>(ec, p, g, first, has_res, has_mask);
    auto run = [&](auto MODEC) {
        constexpr int MODE = decltype(MODEC)::value;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int co = n0 + wn0 + 32 * j + r;
                const bool cok = co < p.Cb;
                const float bv = (p.bias && first && cok) ? p.bias[co] : 0.f;
                float a_[16];
#pragma unroll
                for (int e = 0; e < 16; ++e) a_[e] = acc[i][j][e];
                epi_block<16, MODE>(ec, a_, m0 + wm0 + 32 * i + 4 * h, co, cok, bv);
            }
    };
    epi_dispatch<0, 0>(p, has_res, has_mask, run);
}

// -------------------------------------------------------------------------------------------------
// fp16 weight gradient: C[co][j] = sum over pixels of dY[pixel][co] * x~[pixel][j], j = (tap, ci); 128 x 128 tile, 32 pixels per
// K step, pixel slices combined with float atomics (as conv_wgrad_kernel).  Both LDS images are [pixel][128 channels] in halves
// (256-byte rows) with the 16-byte chunks of a row XOR-swizzled by the row (cdna_hip_programming.md T10 form (b)):
//     off(row, chunk) = 256 * row + 16 * (chunk ^ (((row & 3) << 2) | ((row >> 2) & 3)))
// A lane stages a float4 (4 channels of one pixel) as 4 halves = half a chunk; an MFMA operand (32 channels x 16 pixels, 8 pixels
// of one channel per lane) is two ds_read_b64_tr_b16 per lane: per group of 16 lanes a block of 4 pixels x 16 channels comes back
// transposed, lane i of the group receiving channel i of the four pixels.
// -------------------------------------------------------------------------------------------------
__device__ __forceinline__ int wg16_off(int row, int chunk) {   // byte offset inside one [32][128]-half image
    return 256 * row + 16 * (chunk ^ (((row & 3) << 2) | ((row >> 2) & 3)));
}

template <bool FASTB, bool SAT = true>
__global__ __launch_bounds__(256, 2) void conv_wgrad_f16_kernel(const WgP p) {
    constexpr int BM = 128, BN = 128, TM = 2, TN = 2, WBK = 32;
    constexpr int IMG = WBK * 256;                       // bytes of one image
    constexpr int PER = 4;                               // float4 per thread, operand and K step: rows ak + 8 i
    __shared__ __attribute__((aligned(16))) char lds[4 * IMG];   // A0, A1, B0, B1
    const Geo& g = p.g;
    const int t = threadIdx.x;
    int bx, by, bz;
    if (!wgrad_block(p, bx, by, bz)) return;
    const int j0 = bx * BN, co0 = by * BM;
    const int mbeg = bz * p.mper, mend = min(p.M, mbeg + p.mper);
    const int He = g.Hin << g.ups, We = g.Win << g.ups;
    const int cq = t & 31, ak = t >> 5;                  // channel quad of the 128-wide row, first pixel row
    const int ac = cq * 4;
    const int j = j0 + ac;
    const bool b_jok = j < p.Kcols;
    const int tap = b_jok ? j / p.Cin : 0;
    const int ci = b_jok ? j - tap * p.Cin : 0;
    const int ta = tap / g.Tw, tb = tap - ta * g.Tw;
    const int dh = ta + g.off_y, dw = tb + g.off_x;
    const bool do_bias = p.bias_slabs != nullptr && bx == 0;
    const int b_bias = ((g.off_y < 0 ? -g.off_y : 0) * g.Win + (g.off_x < 0 ? -g.off_x : 0)) * p.Cin * 4;
    const __amdgpu_buffer_rsrc_t rxb = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)p.x - b_bias), 0, p.x_bytes + (unsigned)b_bias, 0x00020000);
    unsigned a_v[PER], b_l[PER];
    int b_dx[PER], b_dy[PER], st_off[PER];
    const bool a_cok = co0 + ac < p.Cout;                // Cout % 4 == 0: the whole quad
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int row = ak + 8 * i;
        a_v[i] = a_cok ? (unsigned)((row * p.Cout + co0 + ac) * 4) : BUF_OOB;
        b_dy[i] = (row >> g.logW) * g.s_in + dh;
        b_dx[i] = (row & (g.W - 1)) * g.s_in + dw;
        b_l[i] = b_jok ? (unsigned)(((b_dy[i] * g.Win + b_dx[i]) * p.Cin + ci) * 4 + b_bias) : BUF_OOB;
        st_off[i] = wg16_off(row, cq >> 1) + 8 * (cq & 1);
    }
    f32x4 ra[PER], rb[PER];
    float bsum[4] = {0.f, 0.f, 0.f, 0.f};
    auto load_tiles = [&](int mb) {
        const int left = mend - mb;
        const __amdgpu_buffer_rsrc_t ra_rs = __builtin_amdgcn_make_buffer_rsrc(
            (void*)(p.dy + (long long)mb * p.Cout), 0, (unsigned)min(left, WBK) * (unsigned)p.Cout * 4u, 0x00020000);
#pragma unroll
        for (int i = 0; i < PER; ++i) ra[i] = buf_load4(ra_rs, a_v[i], 0);
        if constexpr (FASTB) {
            const int n = mb >> (g.logH + g.logW);
            const int oys = ((mb >> g.logW) & (g.H - 1)) * g.s_in, oxs = (mb & (g.W - 1)) * g.s_in;
            const unsigned u = (unsigned)((((n * g.Hin + oys) * g.Win) + oxs) * p.Cin * 4);
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                const bool v = (unsigned)(oys + b_dy[i]) < (unsigned)He && (unsigned)(oxs + b_dx[i]) < (unsigned)We;
                rb[i] = buf_load4(rxb, v ? b_l[i] : BUF_OOB, u);
            }
        } else {
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                const int m = mb + ak + 8 * i;
                const int n = m >> (g.logH + g.logW);
                const int iy = ((m >> g.logW) & (g.H - 1)) * g.s_in + dh;
                const int ix = (m & (g.W - 1)) * g.s_in + dw;
                const bool v = b_jok && m < mend && (unsigned)iy < (unsigned)He && (unsigned)ix < (unsigned)We;
                const unsigned off = (unsigned)((((n * g.Hin + (iy >> g.ups)) * g.Win + (ix >> g.ups)) * p.Cin + ci) * 4 + b_bias);
                rb[i] = buf_load4(rxb, v ? off : BUF_OOB, 0);
            }
        }
    };
    const bool act_a = p.a_slope != 1.0f, act_b = p.pre_slope != 1.0f;
    auto store_tiles = [&](int buf) {
        if (act_a) {
#pragma unroll
            for (int i = 0; i < PER; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) ra[i][e] = __builtin_amdgcn_fmed3f(ra[i][e], ra[i][e] * p.a_slope, p.pos_inf);
        }
        if (do_bias) {
            asm volatile("" ::: "memory");   // a real branch (see conv_wgrad_kernel)
#pragma unroll
            for (int i = 0; i < PER; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) bsum[e] += ra[i][e];
        }
        if (act_b) {
#pragma unroll
            for (int i = 0; i < PER; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) rb[i][e] = __builtin_amdgcn_fmed3f(rb[i][e], rb[i][e] * p.pre_slope, p.pos_inf);
        }
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            *reinterpret_cast<h4_t*>(lds + buf * IMG + st_off[i]) = cvt4_f16<SAT>(ra[i]);
            *reinterpret_cast<h4_t*>(lds + (2 + buf) * IMG + st_off[i]) = cvt4_f16<SAT>(rb[i]);
        }
    };
    // transposed-read addresses: lane = 16 g + 4 q + p of the wave; operand block = 32 channels (16 (g & 1) selects the half),
    // pixels 16 kk + 8 (g >> 1) + 4 rd + q for read rd in {0, 1}; the lane supplies row (pixel), channels c .. c + 3
    const int lane = t & 63, wv = t >> 6, r = lane & 31, h = lane >> 5;
    const int wm0 = (wv >> 1) * 64, wn0 = (wv & 1) * 64;
    const int gg = lane >> 4, qq = (lane >> 2) & 3, pp = lane & 3;
    int a_rd[TM][2], b_rd[TN][2];
#pragma unroll
    for (int rd = 0; rd < 2; ++rd) {
        const int row = 8 * (gg >> 1) + 4 * rd + qq;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int c = wm0 + 32 * i + 16 * (gg & 1) + 4 * pp;
            a_rd[i][rd] = wg16_off(row, c >> 3) + 8 * ((c >> 2) & 1);
        }
#pragma unroll
        for (int jj = 0; jj < TN; ++jj) {
            const int c = wn0 + 32 * jj + 16 * (gg & 1) + 4 * pp;
            b_rd[jj][rd] = wg16_off(row, c >> 3) + 8 * ((c >> 2) & 1);
        }
    }
    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int jj = 0; jj < TN; ++jj)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][jj][e] = 0.f;
    const int nk = (mend > mbeg) ? (mend - mbeg + WBK - 1) / WBK : 0;
    if (nk > 0) {
        load_tiles(mbeg);
        store_tiles(0);
    }
    __syncthreads();
    typedef s16x4 __attribute__((address_space(3))) * lds_s4_ptr;
    auto tr_read = [&](int byte_off) -> h4_t {
        // (16 pixel rows further down = + 4096 bytes: the row's swizzle bits do not change, the offset folds into the immediate)
        return __builtin_bit_cast(h4_t, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4_ptr)(lds + byte_off)));
    };
    auto kstep = [&](int ks, auto BUFC, auto MAINC) {
        constexpr int buf = decltype(BUFC)::value;
        constexpr bool MAIN = decltype(MAINC)::value;
        if (MAIN || ks + 1 < nk) load_tiles(mbeg + (ks + 1) * WBK);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            h8_t a[TM], b[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const h4_t lo = tr_read(buf * IMG + 4096 * kk + a_rd[i][0]), hi = tr_read(buf * IMG + 4096 * kk + a_rd[i][1]);
                a[i] = h8_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            }
#pragma unroll
            for (int jj = 0; jj < TN; ++jj) {
                const h4_t lo = tr_read((2 + buf) * IMG + 4096 * kk + b_rd[jj][0]), hi = tr_read((2 + buf) * IMG + 4096 * kk + b_rd[jj][1]);
                b[jj] = h8_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            }
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int jj = 0; jj < TN; ++jj)
                    acc[i][jj] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[i], b[jj], acc[i][jj], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (MAIN || ks + 1 < nk) store_tiles(buf ^ 1);
        __syncthreads();
    };
    int ks = 0;
    for (; ks + 2 < nk; ks += 2) {
        kstep(ks, std::integral_constant<int, 0>(), std::true_type());
        kstep(ks + 1, std::integral_constant<int, 1>(), std::true_type());
    }
    for (; ks + 1 < nk; ks += 2) {
        kstep(ks, std::integral_constant<int, 0>(), std::false_type());
        kstep(ks + 1, std::integral_constant<int, 1>(), std::false_type());
    }
    if (ks < nk) kstep(ks, std::integral_constant<int, 0>(), std::false_type());

    float* out = p.slabs + (p.atomic ? 0 : (long long)bz * p.Cout * p.Kcols);
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int jj = 0; jj < TN; ++jj) {
            const int col = j0 + wn0 + 32 * jj + r;
            if (col >= p.Kcols) continue;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int co = co0 + wm0 + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * h;
                if (co < p.Cout) {
                    if (p.atomic) atomicAdd(&out[(long long)co * p.Kcols + col], acc[i][jj][e]);
                    else out[(long long)co * p.Kcols + col] = acc[i][jj][e];
                }
            }
        }
    if (do_bias) {   // the images are free after the loop's last barrier: 8 pixel-row phases x 128 channels of fp32 partial sums
        float* red = reinterpret_cast<float*>(lds);
#pragma unroll
        for (int e = 0; e < 4; ++e) red[ak * BM + ac + e] = bsum[e];
        __syncthreads();
        if (t < BM && co0 + t < p.Cout) {
            float sacc = 0.f;
#pragma unroll
            for (int rr = 0; rr < 8; ++rr) sacc += red[rr * BM + t];
            if (p.atomic) atomicAdd(&p.bias_slabs[co0 + t], sacc);
            else p.bias_slabs[(long long)bz * p.Cout + co0 + t] = sacc;
        }
    }
}
