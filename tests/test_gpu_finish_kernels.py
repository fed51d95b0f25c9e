"""The spectral-norm and weight-gradient finish kernels (csrc/spectral.hip) and the column sums of the bias gradients, called
through the C ABI (_lib.load()) one branch at a time, against the fp64 references of tests/finish_ref.py:

  A. gim_spectral_sigma: ragged row chunks, K beyond one block pass, two training rounds and an eval round, a zero weight;
  B. gim_spectral_sigma_batched from a job table built here as the header describes it, and through model_blocks.SNPlan;
  C. gim_wgrad_finish: slab counts on both sides of the unrolled loop's boundary, folds x sigma x destination x bias;
  D. gim_wgrad_finish_batched: one job table whose jobs each reach a named kernel body (the predicate is asserted);
  E. gim_colsum, gim_colsum_acc, gim_colsum2, gim_colsum_grouped at row counts around their loop and split boundaries.

Every output, scratch, tmp and partial buffer has the minimum size the header states and lies between two guard bands of 64
sentinel floats inside one allocation of its own; the bands are asserted untouched after every call.

Two metrics per comparison, both printed before they are asserted (lines "FINISH <group> ..."):
  * relative L2 error < TOL = 3e-5, the suite's bound of an fp32 kernel against fp64 (test_gpu_ops.py, test_gpu_bn_train.py);
  * elementwise |got - ref| <= gamma(m) * scale_i, gamma(m) = m u / (1 - m u), u = 2^-24, m the number of fp32 operations on the
    longest path to the element and scale_i the sum of the absolute values of its terms (the form of _fold_within_bound in
    test_gpu_ops.py).  m per case, derived from the operation and stated where it is used:
      slab sum (C, D without sigma): n_slabs + 4     (n_slabs - 1 additions, three of the fold, its factor, the add into G0);
      column sum (E, bias gradients): rows + 1       (rows - 1 additions, the add into the pre-filled output, one to spare);
      anything behind <g, W> (sigma forms of C, D): n + 8 with n = Cout K K Cin  (n products and additions of the dot product
        in any order; 1/sigma, its square, the two products with u and v, the subtraction, the add into G0).  The scale is built
        from the absolute slab / fold sums, so the n_slabs + 4 operations in front of the dot product are covered: n >= 128 here
        and the dot product's real chain (per-thread loop, block tree, partials) is below 40 operations;
      power iteration (A, B): per stage, from the vectors the device fed that stage (finish_ref.power_iteration_stages)."""
import numpy as np
import pytest
import torch

from oracle import portable_fill as pf
from tests import finish_ref as fr
from tests.helpers import GUARD, JUNK, SENTINEL, TOL, Guarded, Pool, _WORST, _check, _dev_tensor, _report, dev, f32, f64

pytestmark = pytest.mark.gpu


def _lib():
    from optimalstrategiesagainstgenerativeattacks_amd import _lib as L
    return L


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _report_sigma(group, what, got, ref_chain, ref_local, S_chain, S_local, m):
    """sigma against the chained fp64 reference as |delta| / S < TOL (S = sum |u_i W_ij v_j|: with arbitrary u, v sigma is a small
    remainder of cancelling terms), and against u_got^T W v_got within gamma(m) * S."""
    rel = abs(got - ref_chain) / S_chain
    ratio = abs(got - ref_local) / (fr.gamma(m) * S_local)
    w = _WORST.setdefault(group, [0.0, 0.0])
    w[0], w[1] = max(w[0], rel), max(w[1], ratio)
    print("FINISH %s %s: sigma %.7e  |delta| / S %.3e (TOL %.0e)  error / bound %.4f (m = %d)   [group worst so far: %.3e, %.4f]"
          % (group, what, got, rel, TOL, ratio, m, w[0], w[1]))
    assert np.isfinite(got) and rel < TOL and ratio <= 1.0, (what, got, ref_chain, ref_local, rel, ratio)


# ---------------------------------------------------------------------------------------------------------------------
# A / B. power iteration
# ---------------------------------------------------------------------------------------------------------------------
SN_SHAPES = [(1, 1, 1), (4, 1, 3), (65, 7, 1), (130, 24, 3), (450, 12, 3), (72, 130, 3), (512, 40, 1), (3, 64, 9)]    # (Cout, Cin, K)
SN_CHUNKS = {(1, 1, 1): [1], (4, 1, 3): [4], (65, 7, 1): [33, 32], (130, 24, 3): [44, 44, 42], (450, 12, 3): [57] * 7 + [51],
             (72, 130, 3): [36, 36], (512, 40, 1): [64] * 8, (3, 64, 9): [3]}
_SN_INPUTS = {}


def _sn_rows(Cout):
    """(R, rows per chunk) of the W^T u partial sums: R = min(8, ceil(Cout / 64)) chunks of ceil(Cout / R) rows (include/gim_hip.h)."""
    R = min(8, (Cout + 63) // 64)
    return R, (Cout + R - 1) // R


def _sn_inputs(shape):
    """fp32 W [Cout][K][K][Cin] = normal / sqrt(Cin K K) and normalised random u, v, made once."""
    if shape not in _SN_INPUTS:
        Cout, Cin, K = shape
        t = "finish_sn%s" % (shape,)
        W = f32(pf.normal(t + "w", (Cout, K, K, Cin)) / np.sqrt(Cin * K * K))
        u, v = pf.normal(t + "u", (Cout,)), pf.normal(t + "v", (Cin * K * K,))
        _SN_INPUTS[shape] = (W, f32(u / np.linalg.norm(u)), f32(v / np.linalg.norm(v)))
    return _SN_INPUTS[shape]


def test_row_chunks_of_the_shapes_are_the_ragged_ones():
    for shape, chunks in SN_CHUNKS.items():
        R, per = _sn_rows(shape[0])
        assert [min(shape[0], (r + 1) * per) - r * per for r in range(R)] == chunks, shape
    assert 72 * 130 * 9 // 72 > 1024 and 64 * 81 == 5184


class _SnRounds:
    """The chained fp64 reference of one conv and the comparison of a device round with it (shared by A and B)."""

    def __init__(self, group, shape, W, u0, v0):
        self.group, self.shape, self.W = group, shape, f64(W)
        self.u, self.v = f64(u0), f64(v0)          # chained fp64 state
        self.dev_u, self.dev_v = f64(u0), f64(v0)  # what the device holds (fp32 values)

    def compare(self, rnd, training, sigma, u_used, v_used):
        """sigma, u_used, v_used: what the device returned for this round (numpy).  Vectors: L2 against the chained reference (it
        carries the earlier rounds' rounding), the elementwise bound against the reference of the stage alone."""
        Cout, Cin, K = self.shape
        what = "%s round %d %s" % (self.shape, rnd, "train" if training else "eval")
        s_ref, self.u, self.v, S = fr.power_iteration(self.W, self.u, self.v, training)
        m_sigma = 2 * Cin * K * K + 2 * Cout    # K products and additions per row of W v, Cout products and additions of u . t
        if training:
            v_ref, v_b, u_ref, u_b, s_loc, S_loc = fr.power_iteration_stages(self.W, self.dev_u, v_used, u_used)
            for name, got, chain, local, bound in (("v", v_used, self.v, v_ref, v_b), ("u", u_used, self.u, u_ref, u_b)):
                _check(self.group, what + " " + name, got, local, bound=bound, l2_ref=chain)
            self.dev_u, self.dev_v = f64(u_used), f64(v_used)
        else:
            assert np.array_equal(u_used, self.dev_u) and np.array_equal(v_used, self.dev_v), what + ": eval must use the stored u, v"
            M = fr.weight_mat(self.W)
            s_loc, S_loc = float(self.dev_u @ (M @ self.dev_v)), float(np.abs(self.dev_u) @ (np.abs(M) @ np.abs(self.dev_v)))
        _report_sigma(self.group, what, float(sigma), s_ref, s_loc, S, S_loc, m_sigma)


@pytest.mark.parametrize("shape", SN_SHAPES)
def test_spectral_sigma(shape):
    lib = _lib().load()
    Cout, Cin, K = shape
    Kc = Cin * K * K
    W, u0, v0 = _sn_inputs(shape)
    pool = Pool()
    w, u, v = pool.new("w", W.size, W), pool.new("u", Cout, u0), pool.new("v", Kc, v0)
    sigma, u_out, v_out = pool.new("sigma", 1), pool.new("u_out", Cout), pool.new("v_out", Kc)
    scratch = pool.new("scratch", 9 * Kc + Cout)
    ref = _SnRounds("A", shape, W, u0, v0)
    for rnd, training in enumerate((1, 1, 0)):
        for g in (sigma, u_out, v_out, scratch):
            g.fill()
        before = (u.t.clone(), v.t.clone())
        _lib().check(lib.gim_spectral_sigma(w.ptr, u.ptr, v.ptr, sigma.ptr, u_out.ptr, v_out.ptr, scratch.ptr, Cout, Cin, K, training,
                                            _stream()), "spectral_sigma")
        pool.check("gim_spectral_sigma %s round %d" % (shape, rnd))
        assert torch.equal(u.t, u_out.t) and torch.equal(v.t, v_out.t), "u_out / v_out are copies of the vectors used"
        if not training:
            assert torch.equal(u.t, before[0]) and torch.equal(v.t, before[1]), "eval leaves u, v as they were"
        assert torch.equal(w.t, _dev_tensor(W))
        ref.compare(rnd, training, sigma.np()[0], u_out.np(), v_out.np())


def test_spectral_sigma_of_a_zero_weight_is_zero():
    """F.normalize(0, eps) = 0 / eps = 0 and the kernel's 0 * (1 / max(0, 1e-12)) = 0: sigma, u and v are exactly 0."""
    lib = _lib().load()
    Cout, Cin, K = 65, 7, 3
    Kc = Cin * K * K
    _, u0, _ = _sn_inputs((65, 7, 1))
    v0 = pf.normal("finish_zero_v", (Kc,))
    pool = Pool()
    w, u, v = pool.new("w", Cout * Kc, np.zeros(Cout * Kc)), pool.new("u", Cout, u0), pool.new("v", Kc, v0 / np.linalg.norm(v0))
    sigma, u_out, v_out, scratch = pool.new("sigma", 1), pool.new("u_out", Cout), pool.new("v_out", Kc), pool.new("scratch", 9 * Kc + Cout)
    _lib().check(lib.gim_spectral_sigma(w.ptr, u.ptr, v.ptr, sigma.ptr, u_out.ptr, v_out.ptr, scratch.ptr, Cout, Cin, K, 1, _stream()),
                 "spectral_sigma")
    pool.check("gim_spectral_sigma, zero weight")
    for g in (sigma, u, v, u_out, v_out):
        assert not g.np().any(), g.name
    assert fr.power_iteration(np.zeros((Cout, K, K, Cin)), u0, v0 / np.linalg.norm(v0), True, degenerate_ok=True)[0] == 0.0


def test_spectral_sigma_batched_from_a_table_built_as_the_header_says():
    """All eight shapes in ONE job table, one call per round.  (No bit-equality with the sequential entry point: the two vnorm
    kernels reduce in different orders.)  out_base holds, per job, sigma, u, v and 10 K + Cout floats of scratch, each section
    between sentinel gaps."""
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    L = _lib()
    lib = L.load()
    pool = Pool()
    jobs = (L.GimSnJob * len(SN_SHAPES))()
    cols, rows, sections, bufs, refs = [], [], [], [], []
    off = GUARD

    def take(n):
        nonlocal off
        o = off
        off += n + GUARD
        return o
    for j, shape in enumerate(SN_SHAPES):
        Cout, Cin, K = shape
        Kc = Cin * K * K
        W, u0, v0 = _sn_inputs(shape)
        w, u, v = pool.new("w%d" % j, W.size, W), pool.new("u%d" % j, Cout, u0), pool.new("v%d" % j, Kc, v0)
        o_s, o_u, o_v, o_scr = take(1), take(Cout), take(Kc), take(10 * Kc + Cout)
        jobs[j] = (w.ptr, u.ptr, v.ptr, o_s, o_u, o_v, o_scr, Cout, Cin, K, 0)
        R, per = _sn_rows(Cout)
        cols += [(j, xb, r, per) for xb in range((Kc + 255) // 256) for r in range(R)]
        rows += [(j, rb) for rb in range((Cout + 3) // 4)]
        sections.append((o_s, o_u, o_v, o_scr))
        bufs.append((w, u, v))
        refs.append(_SnRounds("B", shape, W, u0, v0))
    total = off
    used = torch.zeros(total, dtype=torch.bool)
    for (Cout, Cin, K), (o_s, o_u, o_v, o_scr) in zip(SN_SHAPES, sections):
        Kc = Cin * K * K
        for o, n in ((o_s, 1), (o_u, Cout), (o_v, Kc), (o_scr, 10 * Kc + Cout)):
            used[o:o + n] = True
    gaps = (~used).to(dev())
    assert int(gaps.sum()) == GUARD * (4 * len(SN_SHAPES) + 1)
    out = torch.empty(total, dtype=torch.float32, device=dev())
    tab = ops._DeviceTable(jobs, cols, rows)
    tab.use_on_current_stream()
    d_jobs, d_cols, d_rows = tab.ptrs
    for rnd, training in enumerate((1, 1, 0)):
        out.fill_(SENTINEL)
        before = [(u.t.clone(), v.t.clone()) for _, u, v in bufs]
        L.check(lib.gim_spectral_sigma_batched(d_jobs, len(SN_SHAPES), d_cols, len(cols), d_rows, len(rows), out.data_ptr(), training,
                                               _stream()), "spectral_sigma_batched")
        pool.check("gim_spectral_sigma_batched round %d" % rnd)
        assert bool((out[gaps] == SENTINEL).all()), "a section of out_base was overrun in round %d" % rnd
        host = out.double().cpu().numpy()
        for (Cout, Cin, K), (o_s, o_u, o_v, _), (w, u, v), ref, (bu, bv) in zip(SN_SHAPES, sections, bufs, refs, before):
            Kc = Cin * K * K
            assert torch.equal(u.t, out[o_u:o_u + Cout]) and torch.equal(v.t, out[o_v:o_v + Kc])
            if not training:
                assert torch.equal(u.t, bu) and torch.equal(v.t, bv)
            ref.compare(rnd, training, host[o_s], host[o_u:o_u + Cout], host[o_v:o_v + Kc])


def test_sn_plan_table_agrees_with_the_device_row_chunks():
    """model_blocks.SNPlan._build's tab_cols against the device's R for ragged Cout: the eight shapes as SNConv2d modules,
    run(2, True), every popped (sigma, u, v) against the reference."""
    from optimalstrategiesagainstgenerativeattacks_amd import model_blocks as mb
    convs, refs = [], []
    for shape in SN_SHAPES:
        Cout, Cin, K = shape
        W, u0, v0 = _sn_inputs(shape)
        c = mb.SNConv2d(Cin, Cout, K, padding=(K - 1) // 2)
        with torch.no_grad():
            c.weight_orig.copy_(torch.from_numpy(W).permute(0, 3, 1, 2))
            c.weight_u.copy_(torch.from_numpy(u0))
            c.weight_v.copy_(torch.from_numpy(v0))
        c = c.to(dev())
        assert torch.equal(c.weight_orig.detach().permute(0, 2, 3, 1).contiguous().cpu(), torch.from_numpy(W))
        convs.append(c)
        refs.append(_SnRounds("B", shape, W, u0, v0))
    plan = mb.SNPlan(convs)
    plan.run(2, True)
    torch.cuda.synchronize()
    for c, ref in zip(convs, refs):
        assert len(c._sn_queue) == 2
        for rnd in range(2):
            sigma, u_s, v_s = (t.double().cpu().numpy() for t in c._sn_queue[rnd][:3])
            ref.compare(rnd, 1, sigma[0], u_s, v_s)
        assert torch.equal(c.weight_u, c._sn_queue[1][1]) and torch.equal(c.weight_v, c._sn_queue[1][2])


# ---------------------------------------------------------------------------------------------------------------------
# shared: a weight with a real spectral state
# ---------------------------------------------------------------------------------------------------------------------
def _spectral_state(tag, Cout, Cin, K):
    """fp32 (W, sigma, u, v): W = normal / sqrt(Cin K K), u and v after two fp64 training rounds, sigma = u^T W v of the rounded
    vectors' fp64 values rounded to fp32 (well conditioned after the rounds)."""
    W = f32(pf.normal(tag + "w", (Cout, K, K, Cin)) / np.sqrt(Cin * K * K))
    u, v = pf.normal(tag + "u", (Cout,)), pf.normal(tag + "v", (Cin * K * K,))
    u, v = u / np.linalg.norm(u), v / np.linalg.norm(v)
    for _ in range(2):
        _, u, v, _ = fr.power_iteration(W, u, v, True)
    u, v = f32(u), f32(v)
    sigma = f32([fr.power_iteration(W, u, v, False)[0]])
    assert sigma[0] > 0.05
    return W, sigma, u, v


# ---------------------------------------------------------------------------------------------------------------------
# C. gim_wgrad_finish, the slab form
# ---------------------------------------------------------------------------------------------------------------------
FIN_SHAPES = {"5x3x3": (5, 3, 3), "16x8x1": (16, 8, 1), "70x6x3": (70, 6, 3), "64x64x3": (64, 64, 3)}
# (shape, n_slabs, fold, sigma, destination, bias)
FIN_CASES = [
    ("5x3x3", 1, 0, 0, "ret", None), ("16x8x1", 2, 0, 1, "ret", "db"), ("70x6x3", 3, 0, 0, "acc", "acc_db"),
    ("64x64x3", 4, 0, 1, "acc", None), ("5x3x3", 13, 0, 1, "ret", "acc_db"), ("70x6x3", 17, 0, 0, "ret", "db"),
    ("16x8x1", 33, 0, 1, "acc", "db"), ("5x3x3", 5, 0, 0, "acc", None), ("70x6x3", 16, 0, 1, "ret", None),
    ("64x64x3", 5, 0, 0, "ret", "db"),
    ("5x3x3", 2, 1, 0, "ret", None), ("16x8x1", 5, 1, 1, "acc", "db"), ("70x6x3", 13, 1, 1, "ret", "acc_db"),
    ("64x64x3", 1, 1, 0, "ret", "db"), ("5x3x3", 16, 1, 1, "acc", None), ("16x8x1", 17, 1, 0, "ret", "acc_db"),
    ("70x6x3", 33, 1, 1, "ret", "db"), ("64x64x3", 3, 1, 1, "acc", "acc_db"),
    ("5x3x3", 3, 2, 1, "ret", None), ("16x8x1", 4, 2, 0, "ret", "db"), ("70x6x3", 16, 2, 1, "acc", "acc_db"),
    ("64x64x3", 2, 2, 1, "ret", None), ("5x3x3", 17, 2, 0, "ret", "acc_db"), ("16x8x1", 33, 2, 1, "acc", "db"),
    ("70x6x3", 1, 2, 0, "ret", None), ("64x64x3", 13, 2, 1, "acc", "db"),
] + [("5x3x3", ns, 0, 0, "ret", "db") for ns in (1, 2, 3, 4, 5, 13, 16, 17, 33)] \
  + [("16x8x1", ns, 0, 1, "ret", None) for ns in (1, 2, 3, 4, 5, 13, 16, 17, 33)]
SLAB_COUNTS = {1, 2, 3, 4, 5, 13, 16, 17, 33}


def test_the_mode_matrix_pairs_every_axis_value_with_every_fold():
    for fold in (0, 1, 2):
        mine = [c for c in FIN_CASES if c[2] == fold]
        assert {c[3] for c in mine} == {0, 1} and {c[4] for c in mine} == {"ret", "acc"}, fold
        assert {c[5] for c in mine} == {None, "db", "acc_db"} and {c[0] for c in mine} == set(FIN_SHAPES), fold
        assert not [c for c in mine if fold and not c[3] and c[4] == "acc"], "that combination is refused (its own test)"
    assert {c[1] for c in FIN_CASES} == SLAB_COUNTS
    # wgrad_sum_kernel: slab group sg = 0..3 starts at slab sg and takes the 16-slab unrolled pass while s + 12 < n_slabs, then the
    # tail.  Per group the counts hold a first pass taken and not taken (13, 16, 17 around sg + 12); 33 takes two passes, and
    # group 0 then a tail of one slab
    for sg in range(4):
        assert {sg + 12 < ns for ns in SLAB_COUNTS} == {True, False} and sg + 16 + 12 < 33 <= sg + 32 + 12
    # 36 864 elements: beyond 64 elements x 512 blocks, so the block cap and the grid stride run; 135: no multiple of 64
    assert 64 * 64 * 9 > 64 * 512 and 5 * 3 * 9 % 64


def _fin_inputs(case):
    shape, ns, fold, sig, dest, bias = case
    Cout, Cin, K = FIN_SHAPES[shape]
    t = "finish_c/%s/%d/%d/" % (shape, ns, fold)
    W, sigma, u, v = _spectral_state("finish_c/%s/" % shape, Cout, Cin, K)
    nsrc = fr.src_size(Cout, Cin, K, fold)
    slabs = f32(pf.normal(t + "slabs", (ns, nsrc)))
    bslabs = f32(pf.normal(t + "bias", (ns, Cout)))
    G0, Gb0 = f32(pf.normal(t + "G0", (Cout, K, K, Cin))), f32(pf.normal(t + "Gb0", (Cout,)))
    return W, sigma, u, v, slabs, bslabs, G0, Gb0


def _fin_call(case, inputs):
    """One gim_wgrad_finish call on fresh buffers -> (rc, dw result tensor, db result tensor or None, acc_dw buffer or None)."""
    lib = _lib().load()
    shape, ns, fold, sig, dest, bias = case
    Cout, Cin, K = FIN_SHAPES[shape]
    n = Cout * K * K * Cin
    W, sigma, u, v, slabs, bslabs, G0, Gb0 = inputs
    pool = Pool()
    d_slabs, d_b = _dev_tensor(slabs), _dev_tensor(bslabs)
    d_w, d_sigma, d_u, d_v = _dev_tensor(W), _dev_tensor(sigma), _dev_tensor(u), _dev_tensor(v)
    dw = pool.new("dw", n)
    acc = pool.new("acc_dw", n, G0) if dest == "acc" else None
    db = pool.new("db", Cout) if bias == "db" else None
    acc_db = pool.new("acc_db", Cout, Gb0) if bias == "acc_db" else None
    n_scratch = (512 if (sig or fold) else 0) + (fr.src_size(Cout, Cin, K, fold) if fold else 0)   # the header's minimum
    scratch = pool.new("scratch", n_scratch) if n_scratch else None
    rc = lib.gim_wgrad_finish(d_slabs.data_ptr(), d_b.data_ptr() if bias else None, ns, d_w.data_ptr() if sig else None,
                              d_sigma.data_ptr() if sig else None, d_u.data_ptr() if sig else None, d_v.data_ptr() if sig else None,
                              dw.ptr, db.ptr if db else None, scratch.ptr if scratch else None, Cout, Cin, K, fold,
                              acc.ptr if acc else None, acc_db.ptr if acc_db else None, _stream())
    pool.check("gim_wgrad_finish %s" % (case,))
    assert torch.equal(d_slabs, _dev_tensor(slabs)) and torch.equal(d_w, _dev_tensor(W)), "inputs are read only"
    return rc, (acc if acc else dw).t, (acc_db or db).t if bias else None, acc


@pytest.mark.parametrize("case", FIN_CASES, ids=lambda c: "%s-s%d-f%d-%s-%s-%s" % (c[0], c[1], c[2], "sn" if c[3] else "plain", c[4], c[5]))
def test_wgrad_finish_slab_form(case):
    shape, ns, fold, sig, dest, bias = case
    Cout, Cin, K = FIN_SHAPES[shape]
    n = Cout * K * K * Cin
    inputs = _fin_inputs(case)
    W, sigma, u, v, slabs, bslabs, G0, Gb0 = inputs
    rc, got_w, got_b, _ = _fin_call(case, inputs)
    _lib().check(rc, "wgrad_finish")
    g, _ = fr.unfold(f64(slabs).sum(0), Cout, Cin, K, fold)
    g_abs, _ = fr.unfold(np.abs(f64(slabs)).sum(0), Cout, Cin, K, fold)
    if sig:
        ref, scale = fr.finish(g, W, sigma[0], u, v, g_abs)
        m = n + 8          # behind <g, W>
    else:
        ref, scale = g, g_abs
        m = ns + 4         # a (folded) slab sum
    if dest == "acc":
        ref, scale = ref + f64(G0), scale + np.abs(f64(G0))
    _check("C", "%s dw" % (case,), got_w.double().cpu().numpy(), ref, scale=scale, m=m)
    if bias:
        ref_b, scale_b = f64(bslabs).sum(0), np.abs(f64(bslabs)).sum(0)
        if bias == "acc_db":
            ref_b, scale_b = ref_b + f64(Gb0), scale_b + np.abs(f64(Gb0))
        _check("C", "%s db" % (case,), got_b.double().cpu().numpy(), ref_b, scale=scale_b, m=ns + 1)   # a column sum of ns rows
    # no float atomics in this entry point: a second call on fresh buffers is bit-identical
    rc2, again_w, again_b, _ = _fin_call(case, inputs)
    assert rc2 == 0 and torch.equal(got_w, again_w) and (got_b is None or torch.equal(got_b, again_b))


@pytest.mark.parametrize("fold", [1, 2])
def test_wgrad_finish_refuses_a_folded_plain_gradient_into_an_accumulator(fold):
    case = ("5x3x3", 3, fold, 0, "acc", None)
    inputs = _fin_inputs(case)
    rc, _, _, acc = _fin_call(case, inputs)
    assert rc != 0
    assert torch.equal(acc.t, _dev_tensor(inputs[6])), "acc_dw must be bit-unchanged"
    assert b"acc_dw" in _lib().load().gim_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# D. gim_wgrad_finish_batched
# ---------------------------------------------------------------------------------------------------------------------
CHUNK = 4096
# name: (case number, (Cout, Cin, K), fold, sigma, bias_src, source offset in floats, gradient it adds into,
#        the body of wgq_reduce_kernel it is meant to reach, the body of wgq_apply_kernel (sigma jobs))
D_JOBS = {
    "1_tile":        (1, (64, 128, 3), 2, 1, 0, 0, "g1", "lds_tile", "rmw16"),
    "2_f2_generic":  (2, (64, 24, 3), 2, 1, 0, 0, "g2", "generic", "rmw16"),
    "3_f1_generic":  (3, (16, 8, 3), 1, 1, 1, 0, "g3", "generic", "rmw16"),
    "4_f3_rows":     (4, (16, 3, 3), 3, 1, 1, 0, "g4", "generic", "atomic"),
    "5_dot16_wrap":  (5, (130, 24, 3), 0, 1, 1, 0, "g5", "dot16", "rmw16"),
    "6_dot16_long":  (6, (8, 512, 3), 0, 1, 0, 0, "g6", "dot16", "rmw16"),
    "7_odd_n":       (7, (5, 3, 3), 0, 1, 1, 0, "g7", "generic", "atomic"),
    "8_misaligned":  (8, (16, 8, 3), 0, 1, 0, 1, "g8", "generic", "atomic"),
    "9a_shared":     (9, (16, 8, 3), 0, 1, 1, 0, "g9", "dot16", "atomic"),
    "9b_shared":     (9, (16, 8, 3), 0, 1, 1, 0, "g9", "dot16", "atomic"),
    "10_plain_rmw":  (10, (10, 512, 1), 0, 0, 1, 0, "g10", "plain_rmw16", None),
    "11a_shared":    (11, (10, 512, 1), 0, 0, 1, 0, "g11", "generic", None),
    "11b_shared":    (11, (10, 512, 1), 0, 0, 1, 0, "g11", "generic", None),
    "12_plain_f1":   (12, (16, 8, 3), 1, 0, 1, 0, "g12a", "generic", None),
    "12_plain_f2":   (12, (16, 8, 3), 2, 0, 0, 0, "g12b", "generic", None),
    "12_plain_f3":   (12, (16, 3, 3), 3, 0, 0, 0, "g12c", "generic", None),
}
D_GROUPS = sorted({j[6] for j in D_JOBS.values()}, key=lambda s: (len(s), s))
D_ATOMIC_GROUPS = {"g9", "g11"}     # several jobs add into one gradient with float atomics: the order varies


def _aligned16(*ptrs):
    return all(p % 16 == 0 for p in ptrs)


def _reduce_body(sn, fold, exclusive, Cout, Cin, n, src, w, grad_w):
    """The branch of wgq_reduce_kernel a job takes (csrc/spectral.hip), restated."""
    if sn and fold == 2 and Cout & 63 == 0 and Cin & 63 == 0:
        return "lds_tile"
    if sn and fold == 0 and n & 3 == 0 and _aligned16(src, w):
        return "dot16"
    if not sn and fold == 0 and exclusive and n & 3 == 0 and _aligned16(src, grad_w):
        return "plain_rmw16"
    return "generic"


def _apply_body(fold, exclusive, Cin, src, tmp, grad_w):
    """The branch of wgq_apply_kernel (sigma jobs only)."""
    return "rmw16" if exclusive and Cin & 3 == 0 and _aligned16(tmp if fold else src, grad_w) else "atomic"


_D_DATA = {}


def _d_data():
    """Host inputs of every job and every gradient, made once: {job: (W, sigma, u, v, src, bias_src)}, {group: (G0, Gb0)}."""
    if not _D_DATA:
        jobs, groups = {}, {}
        for name, (_, (Cout, Cin, K), fold, sn, has_bias, _, grp, _, _) in D_JOBS.items():
            t = "finish_d/%s/" % name
            W, sigma, u, v = _spectral_state("finish_d/w%s/" % ((Cout, Cin, K),), Cout, Cin, K)
            if name == "9b_shared":     # one conv called twice in the pass: the second call's state is one round further
                _, u, v, _ = fr.power_iteration(W, u, v, True)
                u, v = f32(u), f32(v)
                sigma = f32([fr.power_iteration(W, u, v, False)[0]])
                assert not np.array_equal(u, jobs["9a_shared"][2]) and sigma[0] > 0.05
            src = f32(pf.normal(t + "src", (fr.src_size(Cout, Cin, K, fold),)))
            jobs[name] = (W, sigma, u, v, src, f32(pf.normal(t + "bias", (Cout,))))
            if grp not in groups:
                groups[grp] = (f32(pf.normal(t + "G0", (Cout, K, K, Cin))), f32(pf.normal(t + "Gb0", (Cout,))))
        _D_DATA["jobs"], _D_DATA["groups"] = jobs, groups
    return _D_DATA["jobs"], _D_DATA["groups"]


def _d_run():
    """Builds every buffer and the job table afresh, calls gim_wgrad_finish_batched once -> {group: (grad_w, grad_b)} (Guarded),
    {job: (reduce body, apply body)} by the predicates on this run's own pointers."""
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    L = _lib()
    lib = L.load()
    data, gdata = _d_data()
    pool = Pool()
    grads = {g: (pool.new(g + "/grad_w", G0.size, G0), pool.new(g + "/grad_b", Gb0.size, Gb0)) for g, (G0, Gb0) in gdata.items()}
    writers = {g: sum(1 for j in D_JOBS.values() if j[6] == g) for g in D_GROUPS}
    arr = (L.GimWgradJob * len(D_JOBS))()
    tab, tab_sn, bodies, keep = [], [], {}, []
    for j, (name, (_, (Cout, Cin, K), fold, sn, has_bias, src_off, grp, _, _)) in enumerate(D_JOBS.items()):
        W, sigma, u, v, src, bias = data[name]
        n = Cout * K * K * Cin
        assert Cout * (K + 1) ** 2 * Cin < 2 ** 31
        n_chunks = (n + CHUNK - 1) // CHUNK
        d_src = _dev_tensor(np.concatenate([np.full(src_off, JUNK, dtype=np.float32), src]))
        d_bias = _dev_tensor(bias) if has_bias else None
        d_w, d_sigma, d_u, d_v = (_dev_tensor(a) for a in (W, sigma, u, v)) if sn else (None,) * 4
        tmp = pool.new(name + "/tmp", n) if (sn and fold) else None
        partial = pool.new(name + "/partial", n_chunks) if sn else None
        keep += [d_src, d_bias, d_w, d_sigma, d_u, d_v]
        gw, gb = grads[grp]
        exclusive = 1 if writers[grp] == 1 else 0
        p = lambda t: t.data_ptr() if t is not None else None
        src_ptr = d_src.data_ptr() + 4 * src_off
        arr[j] = (src_ptr, p(d_bias), p(d_w), p(d_sigma), p(d_u), p(d_v), tmp.ptr if tmp else None, partial.ptr if partial else None,
                  gw.ptr, gb.ptr, Cout, Cin, K, fold, n_chunks, exclusive)
        blocks = [(j, c) for c in range(n_chunks)]
        tab += blocks
        if sn:
            tab_sn += blocks
        bodies[name] = (_reduce_body(sn, fold, exclusive, Cout, Cin, n, src_ptr, p(d_w) or 0, gw.ptr),
                        _apply_body(fold, exclusive, Cin, src_ptr, tmp.ptr if tmp else 0, gw.ptr) if sn else None)
    table = ops._DeviceTable(arr, tab, tab_sn)
    table.use_on_current_stream()
    d_jobs, d_tab, d_sn = table.ptrs
    L.check(lib.gim_wgrad_finish_batched(d_jobs, len(D_JOBS), d_tab, len(tab), d_sn, len(tab_sn), _stream()), "wgrad_finish_batched")
    pool.check("gim_wgrad_finish_batched")
    return grads, bodies


_D_RUNS = []


def _d_runs():
    """The call and a second one on fresh copies, made once for all tests of this group."""
    if not _D_RUNS:
        _D_RUNS.append(_d_run())
        _D_RUNS.append(_d_run())
    return _D_RUNS


def test_batched_finish_jobs_reach_the_bodies_they_are_meant_for():
    (_, bodies), (_, bodies2) = _d_runs()
    for name, job in D_JOBS.items():
        assert bodies[name] == (job[7], job[8]) == bodies2[name], (name, bodies[name])
    assert {b[0] for b in bodies.values()} == {"lds_tile", "dot16", "plain_rmw16", "generic"}
    assert {b[1] for b in bodies.values()} == {"rmw16", "atomic", None}
    # what the table's "what it reaches" column claims about chunks
    assert (64 * 128 * 9) // CHUNK == 18 and (130 * 216 + CHUNK - 1) // CHUNK == 7 and 130 * 216 - 6 * CHUNK == 3504
    assert CHUNK // 216 in (18, 19) and 512 * 9 > CHUNK and fr.row_pad(3, 3) == 16 and 10 * 512 > CHUNK


@pytest.mark.parametrize("group", D_GROUPS)
def test_batched_finish_adds_every_job_into_its_gradient(group):
    data, gdata = _d_data()
    (grads, _), (grads2, _) = _d_runs()
    G0, Gb0 = gdata[group]
    ref, scale = f64(G0).copy(), np.abs(f64(G0))
    ref_b, scale_b = f64(Gb0).copy(), np.abs(f64(Gb0))
    m, n_bias, names = 0, 0, [n for n, j in D_JOBS.items() if j[6] == group]
    for name in names:
        _, (Cout, Cin, K), fold, sn, has_bias, _, _, _, _ = D_JOBS[name]
        W, sigma, u, v, src, bias = data[name]
        g, g_abs = fr.unfold(src, Cout, Cin, K, fold)
        if sn:
            val, sc = fr.finish(g, W, sigma[0], u, v, g_abs)
            m = max(m, Cout * K * K * Cin + 8)     # behind <g, W>
        else:
            val, sc = g, g_abs
            m = max(m, 1 + 4)                      # a folded "slab sum" of one slab
        ref, scale = ref + val, scale + sc
        if has_bias:
            ref_b, scale_b, n_bias = ref_b + f64(bias), scale_b + np.abs(f64(bias)), n_bias + 1
    m += len(names) - 1                            # one more addition per further job of the gradient
    gw, gb = grads[group]
    _check("D", "%s grad_w" % names, gw.np(), ref, scale=scale, m=m)
    if n_bias:
        _check("D", "%s grad_b" % names, gb.np(), ref_b, scale=scale_b, m=n_bias + 1)    # a column sum of n_bias rows
    else:
        assert torch.equal(gb.t, _dev_tensor(Gb0)), "a job without bias_src leaves grad_b alone"
    if group not in D_ATOMIC_GROUPS:
        assert torch.equal(gw.t, grads2[group][0].t) and torch.equal(gb.t, grads2[group][1].t), "no atomics between jobs: bit-identical"


def test_batched_finish_adds_the_bias_once_whatever_the_chunk_count():
    """Chunk 0 alone adds bias_src: the jobs of 7 and 2 chunks land their bias once (the gradient test above holds them to the
    bound; a bias added per chunk would be off by whole multiples), and jobs without bias_src exist beside them."""
    chunks = {n: (j[1][0] * j[1][1] * j[1][2] ** 2 + CHUNK - 1) // CHUNK for n, j in D_JOBS.items()}
    assert chunks["5_dot16_wrap"] == 7 and D_JOBS["5_dot16_wrap"][4] and chunks["10_plain_rmw"] == 2 and D_JOBS["10_plain_rmw"][4]
    assert chunks["1_tile"] == 18 and not D_JOBS["1_tile"][4] and chunks["6_dot16_long"] == 9 and not D_JOBS["6_dot16_long"][4]
    data, gdata = _d_data()
    (grads, _), _ = _d_runs()
    for name, grp in (("5_dot16_wrap", "g5"), ("10_plain_rmw", "g10")):
        got = grads[grp][1].np()
        once, twice = f64(gdata[grp][1]) + f64(data[name][5]), f64(gdata[grp][1]) + 2 * f64(data[name][5])
        assert np.abs(got - once).max() < 1e-5 < np.abs(got - twice).max(), name


# ---------------------------------------------------------------------------------------------------------------------
# E. column sums
# ---------------------------------------------------------------------------------------------------------------------
COL_ROWS = [1, 3, 4, 5, 12, 13, 16, 17, 64, 65, 4097, 16385, 16640]
COL_C = [1, 63, 64, 65, 130]
_COL = {}


def _col_host():
    """X [16640 + 128][130] (every case reads a corner of it; rows 128.. are the second operand of gim_colsum2) and the two
    pre-filled outputs.  Values are 0.5 + normal: with a zero mean a short column sum cancels by chance (one column of 16 rows
    came out at 2.5e-5 of its absolute sum) and a relative L2 error of a one-column result then measures the input's condition
    number, not the kernel; test_column_sum_inputs_are_well_conditioned holds every case's |scale| / |ref| below 4."""
    if "x" not in _COL:
        _COL["x"] = f32(0.5 + pf.normal("finish_e/x", (max(COL_ROWS) + 128, max(COL_C))))
        _COL["out0"] = f32(0.5 + pf.normal("finish_e/out0", (max(COL_C),)))
        _COL["out1"] = f32(0.5 + pf.normal("finish_e/out1", (max(COL_C),)))
    return _COL


def _col_data():
    d = _col_host()
    if "dev" not in d:
        d["dev"] = torch.from_numpy(d["x"]).to(dev())
    return d


def _col_split(rows):
    """(P, rows per part) of the two-stage column sum, as gim_colsum computes them."""
    P = min(256, (rows + 63) // 64)
    per = (rows + P - 1) // P
    return (rows + per - 1) // per, per


def test_column_sum_row_counts_reach_the_split_edges():
    assert _col_split(16640) == (256, 65) and _col_split(16385) == (253, 65) and 16385 - 252 * 65 == 5
    assert _col_split(4097) == (65, 64) and 4097 - 64 * 64 == 1 and _col_split(65) == (2, 33) and _col_split(64) == (1, 64)
    for rg in range(4):      # the 16-way unrolled row loop (r + 12 < rows) and its tail, per row group
        assert {rg + 12 < r for r in COL_ROWS} == {True, False}


def _col_ref(x, r0, rows, C):
    part = f64(x[r0:r0 + rows, :C])
    return part.sum(0), np.abs(part).sum(0)


def test_column_sum_inputs_are_well_conditioned():
    d = _col_host()
    worst = 0.0
    for rows in COL_ROWS:
        for C in COL_C:
            for r0, o in ((0, d["out0"]), (128, d["out1"])):
                if r0 and rows > 65:
                    continue
                ref, scale = _col_ref(d["x"], r0, rows, C)
                for add in (0.0, 1.0):
                    r, sc = ref + add * f64(o[:C]), scale + add * np.abs(f64(o[:C]))
                    worst = max(worst, float(np.linalg.norm(sc) / np.linalg.norm(r)))
    print("FINISH E inputs: largest |scale| / |ref| %.3f" % worst)
    assert worst < 4.0


@pytest.mark.parametrize("rows", COL_ROWS)
def test_colsum_and_colsum_acc(rows):
    lib = _lib().load()
    d = _col_data()
    for C in COL_C:
        x = d["dev"][:rows, :C].contiguous()
        ref, scale = _col_ref(d["x"], 0, rows, C)
        results = []
        for rep in range(2):
            pool = Pool()
            out, acc, scratch = pool.new("out", C), pool.new("acc", C, d["out0"][:C]), pool.new("scratch", 256 * C)
            _lib().check(lib.gim_colsum(x.data_ptr(), out.ptr, scratch.ptr, rows, C, _stream()), "colsum")
            pool.check("gim_colsum rows %d C %d" % (rows, C))
            scratch.fill()
            _lib().check(lib.gim_colsum_acc(x.data_ptr(), acc.ptr, scratch.ptr, rows, C, _stream()), "colsum_acc")
            pool.check("gim_colsum_acc rows %d C %d" % (rows, C))
            results.append((out.t.clone(), acc.t.clone()))
        assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])
        _check("E", "colsum rows %d C %d" % (rows, C), results[0][0].double().cpu().numpy(), ref, scale=scale, m=rows + 1)
        _check("E", "colsum_acc rows %d C %d" % (rows, C), results[0][1].double().cpu().numpy(), ref + f64(d["out0"][:C]),
               scale=scale + np.abs(f64(d["out0"][:C])), m=rows + 1)


@pytest.mark.parametrize("rows", [r for r in COL_ROWS if r <= 65])
def test_colsum2(rows):
    lib = _lib().load()
    d = _col_data()
    for C in COL_C:
        a, b = d["dev"][:rows, :C].contiguous(), d["dev"][128:128 + rows, :C].contiguous()
        (ra, sa), (rb, sb) = _col_ref(d["x"], 0, rows, C), _col_ref(d["x"], 128, rows, C)
        for accumulate in (0, 1):
            results = []
            for rep in range(2):
                pool = Pool()
                oa = pool.new("out_a", C, d["out0"][:C] if accumulate else None)
                ob = pool.new("out_b", C, d["out1"][:C] if accumulate else None)
                _lib().check(lib.gim_colsum2(a.data_ptr(), b.data_ptr(), oa.ptr, ob.ptr, rows, C, accumulate, _stream()), "colsum2")
                pool.check("gim_colsum2 rows %d C %d" % (rows, C))
                results.append((oa.t.clone(), ob.t.clone()))
            assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])
            for name, got, ref, sc, o0 in (("a", results[0][0], ra, sa, d["out0"]), ("b", results[0][1], rb, sb, d["out1"])):
                if accumulate:
                    ref, sc = ref + f64(o0[:C]), sc + np.abs(f64(o0[:C]))
                _check("E", "colsum2 %s rows %d C %d accumulate %d" % (name, rows, C, accumulate), got.double().cpu().numpy(), ref,
                       scale=sc, m=rows + 1)


@pytest.mark.parametrize("rows", COL_ROWS)
def test_colsum_grouped(rows):
    """Every channel count, flags bit 0 clear and set, as ten jobs of one table; A is a strided corner of X (sAi = 130, sAk = 1)."""
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    L = _lib()
    lib = L.load()
    d = _col_data()
    ld = d["x"].shape[1]
    results = []
    for rep in range(2):
        pool = Pool()
        outs = [(C, flag, pool.new("out C %d flags %d" % (C, flag), C, d["out0"][:C] if flag else None)) for C in COL_C for flag in (0, 1)]
        arr = (L.GimGemmJob * len(outs))()
        tiles = []
        for j, (C, flag, out) in enumerate(outs):
            arr[j] = (d["dev"].data_ptr(), None, out.ptr, None, rows, C, 0, 0, ld, 1, 0, 0, flag, 0)
            tiles += [(j, 0, jt) for jt in range((C + 63) // 64)]
        table = ops._DeviceTable(arr, tiles)
        table.use_on_current_stream()
        L.check(lib.gim_colsum_grouped(table.ptrs[0], table.ptrs[1], len(tiles), _stream()), "colsum_grouped")
        pool.check("gim_colsum_grouped rows %d" % rows)
        results.append([out.t.clone() for _, _, out in outs])
    for (C, flag, _), got, again in zip(outs, results[0], results[1]):
        assert torch.equal(got, again)
        ref, scale = _col_ref(d["x"], 0, rows, C)
        if flag:
            ref, scale = ref + f64(d["out0"][:C]), scale + np.abs(f64(d["out0"][:C]))
        _check("E", "colsum_grouped rows %d C %d flags %d" % (rows, C, flag), got.double().cpu().numpy(), ref, scale=scale, m=rows + 1)
