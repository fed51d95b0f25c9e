"""GPU parity of the strided training convolution (ops.conv2d_strided; gim_conv2d_strided_fwd / _dgrad / _wgrad) against fp64
F.conv2d(x, w, b, stride=2, padding=(K-1)//2) and its autograd on the same fp32-rounded inputs, in the metric of tests/helpers.relerr.
No tolerance is new: TOL of test_gpu_ops.py for y, dx and dbias, TOL_WGRAD of test_gpu_rect_maps.py for dw.

The shapes are the smallest at which each path can still go wrong: aligned channels with all four dgrad classes and the boundary row
oy == Ho, H != W both ways, a 1 x 1 output (every tap but four in the padding), small maps of many images (position-major rows, split
K), channel counts off the fast paths on either gather side, the 1x1 shortcut with its three empty classes, a partial last tile."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import portable_fill as pf
from tests.helpers import relerr

pytestmark = pytest.mark.gpu

TOL = 3e-5
TOL_WGRAD = 1e-5

# name -> (N, H, W, Cin, Cout, K, bias)
CASES = {
    "fast": (2, 8, 8, 16, 32, 3, False),
    "rect_8x16": (2, 8, 16, 16, 16, 3, False),
    "rect_16x8": (2, 16, 8, 16, 16, 3, False),
    "smallest_2x2": (4, 2, 2, 16, 16, 3, False),
    "many_images_8x8": (32, 8, 8, 64, 64, 3, False),
    "many_images_4x4": (32, 4, 4, 64, 64, 3, False),
    "generic_cin3": (2, 8, 8, 3, 16, 3, False),
    "generic_cout20": (2, 8, 8, 16, 20, 3, False),
    "shortcut_1x1": (2, 8, 8, 16, 32, 1, False),
    "tile_edge": (3, 16, 16, 64, 128, 3, False),
    "bias": (2, 8, 8, 16, 32, 3, True),
}


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def ops_mod():
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    return ops


def rnd(tag, shape, scale=1.0):
    return torch.from_numpy(np.ascontiguousarray(pf.normal(tag, tuple(shape)) * scale)).float()


_REF = {}


def case_data(name):
    """fp32 inputs (x NHWC, w [Cout, K, K, Cin], b or None, dy NHWC) and the fp64 reference {y, dx, dw, db} of one case, computed once;
    dx / y in NHWC, dw in the storage order."""
    if name not in _REF:
        N, H, W, Cin, Cout, K, bias = CASES[name]
        tag = "strided/" + name
        x, dy = rnd(tag + "/x", (N, H, W, Cin)), rnd(tag + "/dy", (N, H // 2, W // 2, Cout))
        w = rnd(tag + "/w", (Cout, K, K, Cin), (K * K * Cin) ** -0.5)
        b = rnd(tag + "/b", (Cout,)) if bias else None
        xr = x.double().permute(0, 3, 1, 2).requires_grad_()
        wr = w.double().permute(0, 3, 1, 2).requires_grad_()
        br = b.double().requires_grad_() if bias else None
        yr = F.conv2d(xr, wr, br, stride=2, padding=(K - 1) // 2)
        grads = torch.autograd.grad(yr, [xr, wr] + ([br] if bias else []), dy.double().permute(0, 3, 1, 2))
        ref = {"y": yr.detach().permute(0, 2, 3, 1), "dx": grads[0].permute(0, 2, 3, 1), "dw": grads[1].permute(0, 2, 3, 1)}
        if bias:
            ref["db"] = grads[2]
        _REF[name] = ((x, w, b, dy), ref)
    return _REF[name]


def run_case(name, param_form=False):
    """One forward + backward through ops.conv2d_strided -> {y, dx, dw, db} (dw in the storage order).  param_form: the weight as a
    [Cout, Cin, K, K] tensor kept channels-last, as a parameter in FusedAdam's bucket is."""
    ops = ops_mod()
    (x, w, b, dy), _ = case_data(name)
    xg = x.to(dev()).requires_grad_()
    if param_form:
        wg = w.to(dev()).permute(0, 3, 1, 2).detach().requires_grad_()
    else:
        wg = w.to(dev()).requires_grad_()
    bg = b.to(dev()).requires_grad_() if b is not None else None
    y = ops.conv2d_strided(xg, wg, bg, stride=2)
    y.backward(dy.to(dev()))
    out = {"y": y.detach(), "dx": xg.grad, "dw": wg.grad.permute(0, 2, 3, 1) if param_form else wg.grad}
    if b is not None:
        out["db"] = bg.grad
    return out


def check_case(name, got):
    _, ref = case_data(name)
    errs = {k: relerr(got[k], ref[k]) for k in ref}
    print("strided %-16s %s  " % (name, CASES[name]) + "  ".join("%s %.2e" % kv for kv in errs.items()))
    for k, e in errs.items():
        assert tuple(got[k].shape) == tuple(ref[k].shape), (name, k)
        assert e < (TOL_WGRAD if k == "dw" else TOL), (name, k, e)


@pytest.mark.parametrize("name", list(CASES))
def test_conv2d_strided_fwd_bwd(name):
    check_case(name, run_case(name))


@pytest.mark.parametrize("K", [1, 3])
def test_stride_1_is_the_plain_convolution(K):
    """stride = 1 through the same entries (the forward's own stride-1 launch, gim_conv2d_dgrad, the weight gradient's gather at stride 1)."""
    ops = ops_mod()
    N, H, W, Cin, Cout = 2, 8, 8, 16, 32
    tag = "strided/s1/%d" % K
    x, dy = rnd(tag + "/x", (N, H, W, Cin)), rnd(tag + "/dy", (N, H, W, Cout))
    w, b = rnd(tag + "/w", (Cout, K, K, Cin), (K * K * Cin) ** -0.5), rnd(tag + "/b", (Cout,))
    xr, wr, br = x.double().permute(0, 3, 1, 2).requires_grad_(), w.double().permute(0, 3, 1, 2).requires_grad_(), b.double().requires_grad_()
    yr = F.conv2d(xr, wr, br, stride=1, padding=(K - 1) // 2)
    gx, gw, gb = torch.autograd.grad(yr, [xr, wr, br], dy.double().permute(0, 3, 1, 2))
    xg, wg, bg = x.to(dev()).requires_grad_(), w.to(dev()).requires_grad_(), b.to(dev()).requires_grad_()
    y = ops.conv2d_strided(xg, wg, bg, stride=1)
    y.backward(dy.to(dev()))
    errs = (relerr(y, yr.permute(0, 2, 3, 1)), relerr(xg.grad, gx.permute(0, 2, 3, 1)), relerr(wg.grad, gw.permute(0, 2, 3, 1)), relerr(bg.grad, gb))
    print("stride 1, K = %d: y %.2e dx %.2e dw %.2e db %.2e" % ((K,) + errs))
    assert errs[0] < TOL and errs[1] < TOL and errs[2] < TOL_WGRAD and errs[3] < TOL


def test_parameter_form_weight():
    """The weight as ops.conv2d takes a parameter ([Cout, Cin, K, K], channels-last): same launches, gradient in the parameter's form."""
    got = run_case("fast", param_form=True)
    check_case("fast", got)
    assert got["dw"].is_contiguous()      # i.e. the returned [Cout, Cin, K, K] gradient is channels-last, like the weight


@pytest.mark.parametrize("name", ["shortcut_1x1", "fast", "many_images_4x4"])
def test_dgrad_writes_every_element_of_dx(name):
    """The entry point itself on a dx pre-filled with NaN: the three classes of a 1x1 convolution that have no tap are zeros, and
    a launch that splits K adds into zeros, not into what the buffer held."""
    from optimalstrategiesagainstgenerativeattacks_amd import _lib
    lib = _lib.load()
    (x, w, _, dy), ref = case_data(name)
    N, H, W, Cin, Cout, K, _ = CASES[name]
    wd, dyd = w.to(dev()), dy.to(dev())
    sh = _lib.GimInferConv(N, H, W, Cin, Cout, K, 2)
    for det in (0, 1):
        dx = torch.full((N, H, W, Cin), float("nan"), device=dev())
        _lib.check(lib.gim_conv2d_strided_dgrad(dyd.data_ptr(), wd.data_ptr(), dx.data_ptr(), ctypes.byref(sh), det,
                                                torch.cuda.current_stream().cuda_stream), "conv2d_strided_dgrad")
        assert bool(torch.isfinite(dx).all()), (name, det)
        assert relerr(dx, ref["dx"]) < TOL, (name, det)
        if K == 1:
            assert not dx[:, 1::2].any() and not dx[:, :, 1::2].any()


def test_wgrad_entry_accumulates_and_clears():
    """gim_conv2d_strided_wgrad directly: accumulate = 0 defines dw / dbias whatever they held, accumulate = 1 adds to them; with and
    without the workspace of the deterministic combine."""
    from optimalstrategiesagainstgenerativeattacks_amd import _lib
    lib = _lib.load()
    (x, _, _, dy), ref = case_data("bias")
    N, H, W, Cin, Cout, K, _ = CASES["bias"]
    xd, dyd = x.to(dev()), dy.to(dev())
    sh = _lib.GimInferConv(N, H, W, Cin, Cout, K, 2)
    nbytes = ctypes.c_int64(0)
    _lib.check(lib.gim_conv2d_strided_wgrad_workspace(ctypes.byref(sh), ctypes.byref(nbytes)), "workspace")
    st = torch.cuda.current_stream().cuda_stream
    for use_ws in (False, True):
        ws = torch.full((nbytes.value // 4,), float("nan"), device=dev()) if use_ws else None
        for acc in (0, 1):
            pre_w = rnd("strided/pre_w", (Cout, K, K, Cin)).to(dev())
            pre_b = rnd("strided/pre_b", (Cout,)).to(dev())
            dw, db = pre_w.clone(), pre_b.clone()
            _lib.check(lib.gim_conv2d_strided_wgrad(dyd.data_ptr(), xd.data_ptr(), dw.data_ptr(), db.data_ptr(), ctypes.byref(sh), acc,
                                                    ws.data_ptr() if use_ws else None, st), "conv2d_strided_wgrad")
            if acc:
                dw, db = dw - pre_w, db - pre_b
            ew, eb = relerr(dw, ref["dw"]), relerr(db, ref["db"])
            print("wgrad entry ws=%d acc=%d: dw %.2e db %.2e" % (use_ws, acc, ew, eb))
            assert ew < TOL_WGRAD and eb < TOL, (use_ws, acc, ew, eb)


def test_strided_operands_beyond_2gib_are_split_over_the_batch():
    """test_gpu_ops.py::test_conv_operands_beyond_2gib_are_split_over_the_batch for the strided entries: x and dx of 2.5 GB are beyond
    one launch's 32-bit buffer offsets, so every entry halves the batch; K = 3 puts all four dgrad classes across the seam, and the
    second half of the weight gradient must ADD to the first - with the float atomics and with the workspace the query reports.
    (The forward entry has no deterministic mode: it never splits K.)  y and dx on both halves and the seam against fp64 F.conv2d
    and its autograd; dw and dbias against an fp64 sum over chunks of 50 images, within the 1e-4 of the plain test's atomic combine."""
    from optimalstrategiesagainstgenerativeattacks_amd import _lib
    lib = _lib.load()
    N, S, C, K = 600, 256, 16, 3
    So = S // 2
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn(N, S, S, C, device=dev(), generator=g)
    dy = torch.randn(N, So, So, C, device=dev(), generator=g)
    w = torch.randn(C, K, K, C, device=dev(), generator=g) * (K * K * C) ** -0.5
    b = torch.randn(C, device=dev(), generator=g)
    assert x.numel() * 4 > 2 ** 31
    st = torch.cuda.current_stream().cuda_stream
    sh = _lib.GimInferConv(N, S, S, C, C, K, 2)
    slices = (slice(0, 2), slice(299, 301), slice(598, 600))      # both halves and the seam
    wr = w.double().cpu().permute(0, 3, 1, 2)

    y = torch.full((N, So, So, C), float("nan"), device=dev())
    _lib.check(lib.gim_conv2d_strided_fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), ctypes.byref(sh), st), "conv2d_strided_fwd")
    dx_ref = {}
    for sl in slices:
        xr = x[sl].double().cpu().permute(0, 3, 1, 2).requires_grad_()
        yr = F.conv2d(xr, wr, b.double().cpu(), stride=2, padding=1)
        e = relerr(y[sl], yr.detach().permute(0, 2, 3, 1))
        print("strided > 2 GiB: y[%d:%d] %.2e" % (sl.start, sl.stop, e))
        assert e < TOL, (sl, e)
        dx_ref[sl.start] = torch.autograd.grad(yr, xr, dy[sl].double().cpu().permute(0, 3, 1, 2))[0].permute(0, 2, 3, 1)
    del y
    for det in (0, 1):
        dx = torch.full((N, S, S, C), float("nan"), device=dev())
        _lib.check(lib.gim_conv2d_strided_dgrad(dy.data_ptr(), w.data_ptr(), dx.data_ptr(), ctypes.byref(sh), det, st), "conv2d_strided_dgrad")
        for sl in slices:
            e = relerr(dx[sl], dx_ref[sl.start])
            print("strided > 2 GiB: det=%d dx[%d:%d] %.2e" % (det, sl.start, sl.stop, e))
            assert e < TOL, (det, sl, e)
        del dx

    # dw[o][a][b][c] = sum dy[n][oy][ox][o] * xpad[n][2 oy + a][2 ox + b][c]
    dw_ref = torch.zeros(C, K, K, C, device=dev(), dtype=torch.float64)
    db_ref = torch.zeros(C, device=dev(), dtype=torch.float64)
    for n0 in range(0, N, 50):
        xp = F.pad(x[n0:n0 + 50].double(), (0, 0, 1, 1, 1, 1))
        dyc = dy[n0:n0 + 50].double()
        for a in range(K):
            for bb in range(K):
                dw_ref[:, a, bb, :] += torch.einsum("nhwo,nhwc->oc", dyc, xp[:, a:a + S:2, bb:bb + S:2])
        db_ref += dyc.sum((0, 1, 2))
    del xp, dyc
    nbytes = ctypes.c_int64(0)
    _lib.check(lib.gim_conv2d_strided_wgrad_workspace(ctypes.byref(sh), ctypes.byref(nbytes)), "conv2d_strided_wgrad_workspace")
    for use_ws in (False, True):
        ws = torch.full((nbytes.value // 4,), float("nan"), device=dev()) if use_ws else None
        dw = torch.full((C, K, K, C), float("nan"), device=dev())
        db = torch.full((C,), float("nan"), device=dev())
        _lib.check(lib.gim_conv2d_strided_wgrad(dy.data_ptr(), x.data_ptr(), dw.data_ptr(), db.data_ptr(), ctypes.byref(sh), 0,
                                                ws.data_ptr() if use_ws else None, st), "conv2d_strided_wgrad")
        ew, eb = relerr(dw, dw_ref), relerr(db, db_ref)
        print("strided > 2 GiB: ws=%d dw %.2e db %.2e" % (use_ws, ew, eb))
        assert ew < 1e-4 and eb < 1e-4, (use_ws, ew, eb)


@pytest.mark.parametrize("name", ["fast", "many_images_8x8", "many_images_4x4", "bias"])
def test_deterministic_mode_is_bit_reproducible(name):
    ops = ops_mod()
    prev = ops.set_deterministic(True)
    try:
        a, b = run_case(name), run_case(name)
    finally:
        ops.set_deterministic(prev)
    for k in a:
        assert torch.equal(a[k], b[k]), (name, k)
    check_case(name, a)


def test_gradients_land_in_the_optimizer_bucket():
    """With a FusedAdam over weight and bias, dw and dbias are added into its flat gradient bucket by the weight-gradient launch:
    autograd gets None and runs no AccumulateGrad add."""
    from torch.profiler import ProfilerActivity, profile

    from optimalstrategiesagainstgenerativeattacks_amd.optim import FusedAdam
    ops = ops_mod()
    (x, w, b, dy), ref = case_data("bias")
    wp = torch.nn.Parameter(w.permute(0, 3, 1, 2).contiguous().to(dev()))      # as nn.Conv2d holds it
    bp = torch.nn.Parameter(b.to(dev()))
    opt = FusedAdam([wp, bp], lr=1e-3)
    dyd = dy.to(dev())
    for det in (False, True):
        prev = ops.set_deterministic(det)
        try:
            opt.zero_grad()
            xg = x.to(dev()).requires_grad_()
            with profile(activities=[ProfilerActivity.CPU]) as prof:
                y = ops.conv2d_strided(xg, wp, bp, stride=2)
                y.backward(dyd)
                torch.cuda.synchronize()
        finally:
            ops.set_deterministic(prev)
        names = [ev.name for ev in prof.events()]
        assert any("ConvStridedFnBackward" in n for n in names), "the profile saw no backward"
        adds = [n for n in names if n in ("aten::add_", "aten::add")]
        assert not adds, adds
        flat = opt.flat_grad()
        lo, hi = flat.data_ptr(), flat.data_ptr() + 4 * flat.numel()
        assert lo <= wp.grad.data_ptr() < hi and lo <= bp.grad.data_ptr() < hi
        o, n = opt._offsets[wp]
        got_w = flat[o:o + n].view(ref["dw"].shape)          # the bucket slice, in the weight's own memory order
        ob, nb = opt._offsets[bp]
        print("bucket det=%d: dw %.2e db %.2e dx %.2e" % (det, relerr(got_w, ref["dw"]), relerr(flat[ob:ob + nb], ref["db"]), relerr(xg.grad, ref["dx"])))
        assert relerr(got_w, ref["dw"]) < TOL_WGRAD and relerr(flat[ob:ob + nb], ref["db"]) < TOL and relerr(xg.grad, ref["dx"]) < TOL
        assert relerr(y, ref["y"]) < TOL


def test_executed_flops_are_the_convolutions_own():
    """The census after one forward + backward of the fast-path case: one launch group per direction, each 2 N Ho Wo Cin Cout 9 - a
    padded 4 x 4 fold would list 16 taps, a stride-1 convolution behind a subsample 36; and the library's own plan of the same
    shape runs 9 taps over the dgrad's classes."""
    from optimalstrategiesagainstgenerativeattacks_amd import _lib
    ops = ops_mod()
    N, H, W, Cin, Cout, K, _ = CASES["fast"]
    with ops.count_flops() as counts:
        run_case("fast")
    cfg = (N, H // 2, W // 2, Cin, Cout, K, 2)
    flops = 2.0 * N * (H // 2) * (W // 2) * Cin * Cout * 9
    assert dict(counts) == {("strided_fwd", cfg): [1, flops], ("strided_dgrad", cfg): [1, flops], ("strided_wgrad", cfg): [1, flops]}, dict(counts)
    out = (ctypes.c_int32 * 16)()
    sh = _lib.GimInferConv(N, H, W, Cin, Cout, K, 2)
    _lib.check(_lib.load().gim_conv2d_strided_plan(ctypes.byref(sh), 1, ctypes.cast(out, ctypes.c_void_p)), "plan")
    assert sum(out[4 * i] for i in range(4)) == 9 * Cout


def test_fp16_matrix_path_is_refused():
    ops = ops_mod()
    (x, w, _, _), _ = case_data("fast")
    ops.set_matrix_path("fp16")
    try:
        with pytest.raises(RuntimeError, match="fp32 matrix path only"):
            ops.conv2d_strided(x.to(dev()), w.to(dev()))
    finally:
        ops.set_matrix_path("fp32")


def test_bad_shapes_are_refused():
    ops = ops_mod()
    x = torch.zeros(2, 8, 8, 16, device=dev())
    for w, kw in ((torch.zeros(32, 3, 3, 8), {}), (torch.zeros(32, 5, 5, 16), {}), (torch.zeros(32, 3, 3, 16), dict(stride=3)),
                  (torch.zeros(32, 3, 3, 16), dict(bias=torch.zeros(8)))):
        kw = {k: (v.to(dev()) if torch.is_tensor(v) else v) for k, v in kw.items()}
        with pytest.raises(RuntimeError):
            ops.conv2d_strided(x, w.to(dev()), **kw)
    with pytest.raises(RuntimeError):
        ops.conv2d_strided(torch.zeros(2, 12, 8, 16, device=dev()), torch.zeros(32, 3, 3, 16, device=dev()))


# ---------------------------------------------------------------------------------------------------- the IR-SE unit, both routes
@pytest.mark.parametrize("cin,depth", [(32, 64), (64, 64)], ids=["in!=depth", "in==depth"])
def test_unit_routes_agree(cin, depth):
    """irse_unit_train on a stride-2 unit (N = 4, 8 x 8), once on the strided launches and once on the stride-1 + subsample route
    (the module flag behind GIM_NO_STRIDED_CONV): output, input gradient and every parameter gradient agree within TOL relative to
    the tensor's max, and the default route issues no subsample for its convolutions.  (64 channels are the fewest a unit's SE
    bottleneck - depth / 16 channels, a multiple of 4 for the ReLU pass - runs with.)"""
    from optimalstrategiesagainstgenerativeattacks_amd import baseline_training as bt
    from optimalstrategiesagainstgenerativeattacks_amd import baselines as bl
    ops = ops_mod()
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(11)
        unit = bl._Unit(cin, depth, 2)
        with torch.no_grad():      # BatchNorm scales / shifts and PReLU slopes off their defaults
            for k, p in unit.named_parameters():
                if p.dim() == 1:
                    p.add_(0.3 * torch.randn_like(p))
    sd = {k: v.clone() for k, v in unit.state_dict().items()}
    tag = "strided/unit/%d_%d" % (cin, depth)
    x, dy = rnd(tag + "/x", (4, 8, 8, cin)).to(dev()), rnd(tag + "/dy", (4, 4, 4, depth)).to(dev())
    calls = []
    real_subsample2 = ops.subsample2

    def counting_subsample2(t):
        calls.append(tuple(t.shape))
        return real_subsample2(t)

    def run(strided):
        unit.load_state_dict(sd)
        u = unit.to(dev())
        for p in u.parameters():
            p.grad = None
        xg = x.clone().requires_grad_()
        prev_flag, prev_det = bt._STRIDED_CONV, ops.set_deterministic(True)
        bt._STRIDED_CONV, ops.subsample2 = strided, counting_subsample2
        del calls[:]
        try:
            out = bt.irse_unit_train(u, xg)
            out.backward(dy)
        finally:
            bt._STRIDED_CONV, ops.subsample2 = prev_flag, real_subsample2
            ops.set_deterministic(prev_det)
        res = {"out": out.detach(), "dx": xg.grad}
        for k, p in u.named_parameters():
            res["grad/" + k] = p.grad.detach().clone()
        return res, list(calls)
    new, new_calls = run(True)
    old, old_calls = run(False)
    assert new_calls == [] and len(old_calls) == (2 if cin != depth else 1), (new_calls, old_calls)
    assert set(new) == set(old) and len(new) > 10
    for k in new:
        scale = float(old[k].abs().max())
        e = float((new[k] - old[k]).abs().max()) / scale
        print("    %-40s %.3e" % (k, e))
        assert e < TOL, (k, e)
