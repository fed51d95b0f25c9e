"""Entry points whose per-call and batched / grouped forms share one device body (csrc/gemm.hip, csrc/conv_igemm.hip), called
through the C ABI (_lib.load()) against fp64 NumPy:

  F. gim_bgemm: batch 2, the four stride combinations, the scalar kernel on ragged tiles with a K tail, the vector kernel, and the
     vector shape on a misaligned A (the scalar kernel again: the same bits);
  G. gim_bgemm_grouped from one job table built as the header describes: store with bias and ldc > N, add onto a pre-filled C, two
     jobs adding into one zeroed C with float atomics;
  H. gim_conv2d_fold_weights per call, bit-equal to gim_conv2d_fold_weights_batched on the same weights.

Outputs lie between guard bands (tests/helpers.py: Guarded, Pool) and hold JUNK before the call.  Bounds, printed before they are
asserted (lines "FINISH F ..."): relative L2 error < TOL = 3e-5, and elementwise |got - ref| <= gamma(m) * scale_i with
  products (F, G): m = 2 K + 2 - K products and K additions on the path to an element (v_mfma_f32_32x32x2_f32 takes two k per
    instruction; each product and each addition is counted as one rounding), the bias and the add onto C or of the second job;
    scale_i = sum_k |a_ik| |b_kj| (+ |bias_j| + |C0_ij|);
  folds (H): test_gpu_ops._fold_within_bound, gamma(3) on the four-term sum."""
import numpy as np
import pytest
import torch

from oracle import portable_fill as pf
from tests.helpers import JUNK, Guarded, Pool, _check, _dev_tensor, dev, f32, f64

pytestmark = pytest.mark.gpu


def _lib():
    from optimalstrategiesagainstgenerativeattacks_amd import _lib as L
    return L


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------------------------------
# F. gim_bgemm
# ---------------------------------------------------------------------------------------------------------------------
BATCH = 2
GEMM_SCALAR, GEMM_VECTOR = (65, 63, 17), (68, 64, 36)     # (M, N, K)
COMBOS = [(ak, bj) for ak in (1, 0) for bj in (1, 0)]     # A k-contiguous or i-contiguous, B j-contiguous or k-contiguous
_GEMM = {}


def _gemm_host(shape):
    """fp32 A [b][M][K], B [b][K][N] (logical order) and the fp64 product with its absolute twin, made once per shape."""
    if shape not in _GEMM:
        M, N, K = shape
        A = f32(pf.normal("twin_f/%s/A" % (shape,), (BATCH, M, K)))
        B = f32(pf.normal("twin_f/%s/B" % (shape,), (BATCH, K, N)))
        _GEMM[shape] = (A, B, np.einsum("bik,bkj->bij", f64(A), f64(B)), np.einsum("bik,bkj->bij", np.abs(f64(A)), np.abs(f64(B))))
    return _GEMM[shape]


def _operand(a, fast_last, offset=0):
    """`a` [b][rows][cols] in device memory as it is (fast_last) or transposed, behind `offset` floats -> (tensor, address, batch
    stride, row stride, column stride) in elements."""
    b, r, c = a.shape
    mem = a if fast_last else a.transpose(0, 2, 1)
    t = _dev_tensor(np.concatenate([np.full(offset, JUNK, dtype=np.float32), f32(mem).reshape(-1)]))
    return (t, t.data_ptr() + 4 * offset, r * c) + ((c, 1) if fast_last else (1, r))


def vector_path(M, N, K, A_ptr, B_ptr, sAb, sAi, sAk, sBb, sBk, sBj):
    """gim_bgemm's choice of the 16-byte kernel (csrc/gemm.hip), restated."""
    ak, bk = sAk == 1, sBk == 1
    va = (K % 4 == 0 and sAi % 4 == 0) if ak else (sAi == 1 and M % 4 == 0 and sAk % 4 == 0)
    vb = (K % 4 == 0 and sBj % 4 == 0) if bk else (sBj == 1 and N % 4 == 0 and sBk % 4 == 0)
    return va and vb and A_ptr % 16 == 0 and B_ptr % 16 == 0 and sAb % 4 == 0 and sBb % 4 == 0


def bgemm_run(shape, combo, a_offset=0):
    """One gim_bgemm call -> (C as a device tensor [b][M][N], whether the vector kernel ran)."""
    M, N, K = shape
    A, B, _, _ = _gemm_host(shape)
    ta, pa, sAb, sAi, sAk = _operand(A, combo[0], a_offset)
    tb, pb, sBb, sBk, sBj = _operand(B, combo[1])
    pool = Pool()
    C = pool.new("C", BATCH * M * N)
    before = (ta.clone(), tb.clone())
    _lib().check(_lib().load().gim_bgemm(pa, pb, C.ptr, BATCH, M, N, K, sAb, sAi, sAk, sBb, sBk, sBj, _stream()), "bgemm")
    pool.check("gim_bgemm %s %s" % (shape, combo))
    assert torch.equal(ta, before[0]) and torch.equal(tb, before[1]), "operands are read only"
    return C.t.clone().view(BATCH, M, N), vector_path(M, N, K, pa, pb, sAb, sAi, sAk, sBb, sBk, sBj)


@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: "A%s_B%s" % ("k" if c[0] else "i", "j" if c[1] else "k"))
def test_bgemm(combo):
    for shape, want_vector in ((GEMM_SCALAR, False), (GEMM_VECTOR, True)):
        M, N, K = shape
        _, _, ref, scale = _gemm_host(shape)
        got, vec = bgemm_run(shape, combo)
        assert vec == want_vector, (shape, combo)
        _check("F", "bgemm %s %s" % (shape, combo), got.double().cpu().numpy(), ref, scale=scale, m=2 * K + 2)
    # 65 x 63: two row and one column tile, both ragged; 17 = one K step of 16 and a tail of 1.  68 x 64: a second row tile of 4
    # rows; 36 = one K step of 32 and a tail of 4
    assert 65 > 64 > 63 and 17 % 16 == 1 and 68 > 64 and 36 % 32 == 4
    moved, vec = bgemm_run(GEMM_VECTOR, combo, a_offset=1)
    assert not vec, "A one float off a 16-byte boundary takes the scalar kernel"
    assert torch.equal(moved, got), "the scalar and the vector kernel add the products of an element in the same order"


# ---------------------------------------------------------------------------------------------------------------------
# G. gim_bgemm_grouped
# ---------------------------------------------------------------------------------------------------------------------
GROUPED_SHAPES = [(65, 63, 17), (8, 130, 512)]
# (name, flags, bias, extra columns of ldc, A k-contiguous, B j-contiguous, the C it writes)
GROUPED_JOBS = [("store", 0, 1, 5, 1, 1, "c0"), ("add", 1, 0, 0, 0, 0, "c1"), ("atomic_a", 2, 0, 0, 1, 0, "c2"), ("atomic_b", 2, 0, 0, 0, 1, "c2")]
_GROUPED = {}


def _grouped_host():
    """{(shape, job): (A [M][K], B [K][N], bias [N] or None)}, {(shape, C): pre-fill [M][ldc] or None = JUNK}, made once."""
    if not _GROUPED:
        ops_, pre = {}, {}
        for shape in GROUPED_SHAPES:
            M, N, K = shape
            for name, flags, bias, pad, _, _, c in GROUPED_JOBS:
                t = "twin_g/%s/%s/" % (shape, name)
                ops_[shape, name] = (f32(pf.normal(t + "A", (M, K))), f32(pf.normal(t + "B", (K, N))),
                                     f32(pf.normal(t + "bias", (N,))) if bias else None)
            pre[shape, "c0"] = None
            pre[shape, "c1"] = f32(pf.normal("twin_g/%s/C1" % (shape,), (M, N)))
            pre[shape, "c2"] = np.zeros((M, N), dtype=np.float32)
        _GROUPED["ops"], _GROUPED["pre"] = ops_, pre
    return _GROUPED["ops"], _GROUPED["pre"]


def grouped_run(only=None):
    """Every job of both shapes in ONE table (`only`: that job name alone), one gim_bgemm_grouped call -> {(shape, C): Guarded}."""
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    L = _lib()
    data, pre = _grouped_host()
    pool = Pool()
    jobs = [(shape, j) for shape in GROUPED_SHAPES for j in GROUPED_JOBS if only in (None, j[0])]
    outs = {}
    for shape, j in jobs:
        M, N, _ = shape
        if (shape, j[6]) not in outs:
            outs[shape, j[6]] = pool.new("%s %s" % (shape, j[6]), M * (N + j[3]), pre[shape, j[6]])
    arr = (L.GimGemmJob * len(jobs))()
    tiles, keep = [], []
    for n, (shape, (name, flags, bias, pad, ak, bj, c)) in enumerate(jobs):
        M, N, K = shape
        A, B, bv = data[shape, name]
        ta, pa, _, sAi, sAk = _operand(A[None], ak)
        tb, pb, _, sBk, sBj = _operand(B[None], bj)
        d_bias = _dev_tensor(bv) if bias else None
        keep += [ta, tb, d_bias]
        arr[n] = (pa, pb, outs[shape, c].ptr, d_bias.data_ptr() if bias else None, M, N, K, N + pad, sAi, sAk, sBk, sBj, flags, 0)
        tiles += [(n, it, jt) for it in range((M + 63) // 64) for jt in range((N + 63) // 64)]
    table = ops._DeviceTable(arr, tiles)
    table.use_on_current_stream()
    L.check(L.load().gim_bgemm_grouped(table.ptrs[0], table.ptrs[1], len(tiles), _stream()), "bgemm_grouped")
    pool.check("gim_bgemm_grouped")
    return outs


def test_bgemm_grouped_from_a_table_built_as_the_header_says():
    data, pre = _grouped_host()
    outs, again = grouped_run(), grouped_run()
    for shape in GROUPED_SHAPES:
        M, N, K = shape
        prod = {}
        for name, *_ in GROUPED_JOBS:
            A, B, _ = data[shape, name]
            prod[name] = (f64(A) @ f64(B), np.abs(f64(A)) @ np.abs(f64(B)))
        bias = f64(data[shape, "store"][2])
        # flags 0: C = A B + bias in the first N of ldc = N + 5 columns; the others keep what they held
        c0 = outs[shape, "c0"].np().reshape(M, N + 5)
        assert (c0[:, N:] == np.float32(JUNK)).all(), "columns beyond N belong to the caller"
        _check("G", "%s store + bias" % (shape,), c0[:, :N], prod["store"][0] + bias, scale=prod["store"][1] + np.abs(bias), m=2 * K + 2)
        # flags 1: C += A B, one writer per element
        _check("G", "%s add" % (shape,), outs[shape, "c1"].np(), f64(pre[shape, "c1"]) + prod["add"][0],
               scale=np.abs(f64(pre[shape, "c1"])) + prod["add"][1], m=2 * K + 2)
        # flags 2: both jobs add into the zeroed C with float atomics
        _check("G", "%s two atomic jobs" % (shape,), outs[shape, "c2"].np(), prod["atomic_a"][0] + prod["atomic_b"][0],
               scale=prod["atomic_a"][1] + prod["atomic_b"][1], m=2 * K + 2)
        # two terms onto zero: either order of the atomics gives the same bits
        for c in ("c0", "c1", "c2"):
            assert torch.equal(outs[shape, c].t, again[shape, c].t), (shape, c)
    assert (8 * 130 * 512, (130 + 63) // 64, 512 // 16) == (532480, 3, 32)   # one row tile of 8 rows, three column tiles, 32 K steps


# ---------------------------------------------------------------------------------------------------------------------
# H. gim_conv2d_fold_weights
# ---------------------------------------------------------------------------------------------------------------------
FOLD_CHUNK, FOLD_CHUNK_CALL = 65536, 4096     # folded elements per block: the batched launch, the per-call launch
# (Cout, Cin, KH, pointer offset in floats)
FOLD_CASES = [(5, 3, 3, 0), (4, 8, 3, 0), (3, 4, 1, 0), (2, 4, 9, 0), (2, 4, 5, 0), (48, 128, 3, 0), (4, 8, 3, 1),
              (5, 12, 9, 0), (7, 9, 9, 0)]    # two blocks per call, the second ragged: 16-byte path, scalar path
_FOLD_W = {}


def _fold_weight(Cout, Cin, K):
    """fp32 W as torch holds it, [Cout][Cin][K][K] (test_gpu_ops._fold_within_bound reads that order), made once."""
    if (Cout, Cin, K) not in _FOLD_W:
        _FOLD_W[Cout, Cin, K] = torch.from_numpy(f32(pf.normal("twin_h/%s" % ((Cout, Cin, K),), (Cout, Cin, K, K))))
    return _FOLD_W[Cout, Cin, K]


def fold_run(case, batched):
    """One fold of W (memory order [Cout][K][K][Cin]) through the per-call or the batched entry -> F as a device tensor; both
    pointers `offset` floats behind a 16-byte boundary."""
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    L = _lib()
    Cout, Cin, K, offset = case
    n = Cout * (K + 1) ** 2 * Cin
    w = _fold_weight(Cout, Cin, K).permute(0, 2, 3, 1).contiguous().numpy()
    d_w = _dev_tensor(np.concatenate([np.full(offset, JUNK, dtype=np.float32), w.reshape(-1)]))
    pool = Pool()
    f = pool.new("f", n + offset)
    w_ptr, f_ptr = d_w.data_ptr() + 4 * offset, f.ptr + 4 * offset
    assert f.ptr % 16 == 0 and d_w.data_ptr() % 16 == 0
    if batched:
        arr = (L.GimFoldJob * 1)()
        arr[0] = (w_ptr, f_ptr, Cout, Cin, K, 0)
        tab = [(0, c) for c in range((n + FOLD_CHUNK - 1) // FOLD_CHUNK)]
        table = ops._DeviceTable(arr, tab)
        table.use_on_current_stream()
        L.check(L.load().gim_conv2d_fold_weights_batched(table.ptrs[0], table.ptrs[1], len(tab), _stream()), "fold_weights_batched")
    else:
        L.check(L.load().gim_conv2d_fold_weights(w_ptr, f_ptr, Cout, Cin, K, _stream()), "fold_weights")
    pool.check("fold %s batched %d" % (case, batched))
    assert bool((f.t[:offset] == JUNK).all()), "the floats in front of f belong to the caller"
    return f.t[offset:].clone()


@pytest.mark.parametrize("case", FOLD_CASES, ids=lambda c: "%dx%dx%d+%d" % c)
def test_fold_weights_per_call_equals_the_batched_fold(case):
    from tests.test_gpu_ops import _fold_within_bound
    Cout, Cin, K, offset = case
    single, batched = fold_run(case, False), fold_run(case, True)
    assert torch.equal(single, batched), case
    assert _fold_within_bound(single, _fold_weight(Cout, Cin, K)), case
    if offset:   # the scalar path of a misaligned pointer adds the same four terms in the same order as the 16-byte one
        assert torch.equal(single, fold_run((Cout, Cin, K, 0), False))


def test_fold_cases_reach_every_path():
    paths = {(Cin % 4 == 0 and not off, K + 1 if K + 1 in (2, 4, 10) else 0) for _, Cin, K, off in FOLD_CASES}
    assert paths == {(False, 4), (True, 4), (True, 2), (True, 10), (True, 0), (False, 10)}     # (16-byte accesses, compile-time taps)
    assert 48 * 128 * 16 == 98304 and FOLD_CHUNK < 98304 < 2 * FOLD_CHUNK and 98304 == 24 * FOLD_CHUNK_CALL
    assert FOLD_CHUNK_CALL < 5 * 12 * 100 < 7 * 9 * 100 < 2 * FOLD_CHUNK_CALL
