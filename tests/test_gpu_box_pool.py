"""Pooled 3x3 convolutions on the box-filtered input (ops._pool_route "box": gim_box2_fwd + gim_conv_shape.pool = 2): forward and weight
gradient run the conv's own 9 taps at stride 2 on p = box2(lrelu(x)) [N, H+1, W+1, Cin]; the input gradient keeps the folded form.
Everything against fp64 autograd of avg_pool2d(conv2d(leaky_relu(x), w / sigma, padding=1), 2) + b (+ res), with the relerr / TOL
yardstick of tests/test_gpu_ops.py::test_conv2d_pool_fold (fp32 product vs fp64 reference, relative L2)."""
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import portable_fill as pf
from tests.helpers import T, relerr, tune_override

pytestmark = pytest.mark.gpu

TOL = 3e-5      # test_gpu_ops.TOL
SLOPE = 0.2


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def nhwc(x):
    return x.detach().permute(0, 2, 3, 1).contiguous().float().to(dev())


def nchw(y):
    return y.detach().permute(0, 3, 1, 2).double().cpu()


def _sn(w, tag):
    """(sigma, u, v) of a spectral-normed weight after two power iterations from seeded vectors (fp64, v in the logical (ci, kh, kw) order)."""
    Wm = w.detach().reshape(w.shape[0], -1)
    g = torch.Generator().manual_seed(zlib.crc32(tag.encode()) & 0xFFFF)
    u = torch.randn(Wm.shape[0], dtype=torch.float64, generator=g)
    u = u / u.norm()
    for _ in range(2):
        v = Wm.t().mv(u)
        v = v / v.norm()
        u = Wm.mv(v)
        u = u / u.norm()
    return u, v


_REF = {}


def reference(case):
    """fp64 leaves (x, w, b, res, u, v, sigma), y and the cotangent r of one case, the leaves holding the gradients of sum(y * r);
    computed once per case and shared by the tests that run it."""
    if case in _REF:
        return _REF[case]
    N, Cin, Cout, H, W, x_act, post, use_res, sn, ks = case
    tag = "boxpool%s" % (case[:5],)
    x = T(pf.normal(tag + "x", (N, Cin, H, W))).requires_grad_()
    w = T(pf.normal(tag + "w", (Cout, Cin, 3, 3)) / np.sqrt(Cin * 9)).requires_grad_()
    b = T(pf.normal(tag + "b", (Cout,))).requires_grad_()
    res = T(pf.normal(tag + "r", (N, Cout, H // 2, W // 2))).requires_grad_() if use_res else None
    if sn:      # sigma = u^T W v differentiated w.r.t. W with u, v constant: the spectral term of the finish
        u, v = _sn(w, tag)
        sigma = torch.dot(u, w.reshape(Cout, -1).mv(v))
    else:       # a plain 1 / sigma scaling (u = v = 0 on the product side)
        u, v, sigma = torch.zeros(Cout, dtype=torch.float64), torch.zeros(Cin * 9, dtype=torch.float64), torch.tensor(1.3, dtype=torch.float64)
    y = F.avg_pool2d(F.conv2d(F.leaky_relu(x, SLOPE), w / sigma, None, padding=1), 2) + b.view(1, -1, 1, 1)
    if use_res:
        y = y + res
    r = T(pf.uniform(tag + "dy", tuple(y.shape)))
    (y * r).sum().backward()
    _REF[case] = (x, w, b, res, u, v, sigma.detach(), y.detach(), r)
    return _REF[case]


def run_product(ops, case, box=True):
    """The case through ops.conv2d_post_act -> {name: NCHW fp64 cpu tensor}, the counted launches, and whether y was stored activated."""
    N, Cin, Cout, H, W, x_act, post, use_res, sn, ks = case
    x, w, b, res, u, v, sigma, _, r = reference(case)
    xg = nhwc(F.leaky_relu(x, SLOPE) if x_act else x).requires_grad_()
    wg = w.detach().float().to(dev()).contiguous(memory_format=torch.channels_last).requires_grad_()
    bg = b.detach().float().to(dev()).requires_grad_()
    rg = nhwc(res).requires_grad_() if use_res else None
    sg = sigma.reshape(1).float().to(dev())
    ug = u.float().to(dev())
    vg = v.float().to(dev())
    g = ops.ConvGeom.of(xg, wg, 0, SLOPE, True, False, bg, rg, x_act)
    prev = ops._BOX_POOL
    ops._BOX_POOL = box
    try:
        with tune_override(ops, g.box() if box else g, {"fwd": (0, ks)} if ks else None), ops.count_flops() as counts:
            yg, act = ops.conv2d_post_act(xg, wg, bg, rg, sg, ug, vg, 0, SLOPE, pool=True, post_slope=post, x_act=x_act)
            (yg * nhwc(r)).sum().backward()     # ConvFn.backward takes the cotangent as the gradient w.r.t. the RAW y
        assert not ops.wgrad_queue.jobs
    finally:
        ops._BOX_POOL = prev
    out = {"y": nchw(yg), "dx": nchw(xg.grad), "dw": wg.grad.double().cpu(), "db": bg.grad.double().cpu()}
    if use_res:
        out["dres"] = nchw(rg.grad)
    return out, dict(counts), act


def took_box(counts):
    kinds = {kind for (kind, cfg) in counts if kind != "bgemm" and cfg[7] == 2}
    folded = {kind for (kind, cfg) in counts if kind != "bgemm" and cfg[7] == 1}
    return kinds == {"fwd", "wgrad"} and folded == {"dgrad"}


CASES = [
    # N, Cin, Cout, H, W, x_act, post_slope, res, spectral term (u, v != 0), forced split-K of the forward
    (2, 16, 32, 8, 8, False, 1.0, True, False, 0),
    (5, 128, 128, 2, 2, True, 1.0, True, False, 0),        # p is 3x3, one output pixel
    (3, 32, 48, 4, 16, False, SLOPE, False, True, 0),      # non-square, ragged Cout, activated output, spectral term
    (1, 16, 16, 16, 4, True, SLOPE, True, False, 0),       # non-square the other way, x stored activated
    (40, 32, 32, 8, 8, False, 1.0, True, False, 0),        # >= 32 images on a small map (the fold goes position-major here)
    (2, 64, 80, 32, 32, True, SLOPE, True, False, 0),      # large tiles, Cout not a tile multiple
    (3, 128, 64, 16, 16, False, SLOPE, False, False, 3),   # split-K forward: raw output (no activated store), box2_fwd applies the LeakyReLU
]


def box_fwd_ksplit(ops, case):
    """K slices of the 9-tap forward launch of a case, asked from the library (gim_conv_launch_plan out[3])."""
    import ctypes

    from optimalstrategiesagainstgenerativeattacks_amd import _lib
    N, Cin, Cout, H, W, ks = case[:5] + case[9:]
    sh = ops._shape(N, H, W, Cin, Cout, 3, 0, 1.0, 2, 0, 0)
    sh.tune_ksplit = ks
    out = (ctypes.c_int32 * 8)()
    _lib.check(_lib.load().gim_conv_launch_plan(ctypes.byref(sh), 0, ctypes.cast(out, ctypes.c_void_p)), "conv_launch_plan")
    return out[3]


def test_cases_reach_both_store_regimes():
    """Of the cases that ask for an activated output, some launch one K slice (the epilogue activates) and some split K (raw output)."""
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    splits = {box_fwd_ksplit(ops, c) > 1 for c in CASES if c[6] != 1.0}
    assert splits == {False, True}
    assert box_fwd_ksplit(ops, CASES[-1]) == 3


@pytest.mark.parametrize("case", CASES, ids=[str(c) for c in CASES])
def test_box_route_vs_fp64(case):
    """y, dx, dw, db, dres of the box route against fp64 autograd; the counted launches say that forward and wgrad ran the 9-tap
    geometry (pool = 2) and the input gradient the fold."""
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    x, w, b, res, u, v, sigma, y, r = reference(case)
    got, counts, act = run_product(ops, case)
    assert took_box(counts), counts
    post = case[6]
    assert act == (post != 1.0 and box_fwd_ksplit(ops, case) == 1), "an activated store goes with a one-slice launch only"
    ref = {"y": F.leaky_relu(y, post) if act else y, "dx": x.grad, "dw": w.grad, "db": b.grad}
    if res is not None:
        ref["dres"] = res.grad
    errs = {k: relerr(got[k], ref[k]) for k in ref}
    print("box route %s: %s" % (case, " ".join("%s %.2e" % kv for kv in errs.items())))
    for k, e in errs.items():
        assert e < TOL, (k, e)


@pytest.mark.parametrize("case", [CASES[0], CASES[2], CASES[5]], ids=[str(c) for c in (CASES[0], CASES[2], CASES[5])])
def test_box_route_vs_fold_route(case):
    """The two routes on identical inputs: outputs and all gradients within the same bound of each other."""
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    a, ca, _ = run_product(ops, case, box=True)
    f, cf, _ = run_product(ops, case, box=False)
    assert took_box(ca) and not any(cfg[7] == 2 for (kind, cfg) in cf if kind != "bgemm")
    errs = {k: relerr(a[k], f[k]) for k in f}
    print("box vs fold %s: %s" % (case, " ".join("%s %.2e" % kv for kv in errs.items())))
    for k, e in errs.items():
        assert e < TOL, (k, e)


@pytest.mark.parametrize("shape", [(3, 2, 2, 16), (2, 4, 16, 20)], ids=str)
@pytest.mark.parametrize("slope", [1.0, SLOPE])
def test_box2_fwd(shape, slope):
    """gim_box2_fwd alone against avg_pool2d(pad(lrelu(x), 1), 2, stride=1) in fp64 on the fp32-rounded input.  Bound, relative to
    m = max |x|: three additions, each rounded at <= 2^-24 of a partial sum of <= 4 m, times the exact factor 1/4 (3 * 2^-24 m), and
    four slope products rounded at 2^-24 m each with the fp32 slope off by < 2^-26 relative, times 1/4 (< 1.3 * 2^-24 m): 5 * 2^-24 m."""
    from optimalstrategiesagainstgenerativeattacks_amd import _lib
    N, H, W, C = shape
    x = T(pf.normal("box2%s" % (shape,), (N, C, H, W))).float().double()
    ref = F.avg_pool2d(F.pad(F.leaky_relu(x, slope), (1, 1, 1, 1)), 2, stride=1)
    xg = nhwc(x)
    p = torch.full((N, H + 1, W + 1, C), float("nan"), device=dev())
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(_lib.load().gim_box2_fwd(xg.data_ptr(), p.data_ptr(), N, H, W, C, slope, st), "box2_fwd")
    err = float((nchw(p) - ref).abs().max())
    bound = 5 * 2.0 ** -24 * float(x.abs().max())
    print("box2_fwd %s slope %g: max abs err %.2e (bound %.2e)" % (shape, slope, err, bound))
    assert err <= bound


def test_box_route_is_bit_reproducible_in_deterministic_mode():
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    case = (3, 32, 48, 16, 16, False, 1.0, True, True, 0)
    prev = ops.set_deterministic(True)
    try:
        a, ca, _ = run_product(ops, case)
        b, _, _ = run_product(ops, case)
    finally:
        ops.set_deterministic(prev)
    assert took_box(ca), ca
    for k in a:
        assert torch.equal(a[k], b[k]), k
    x, w, bb, res, u, v, sigma, y, r = reference(case)
    assert relerr(a["y"], y) < TOL and relerr(a["dw"], w.grad) < TOL and relerr(a["dx"], x.grad) < TOL


@pytest.mark.parametrize("form", ["proj", "r1"])
def test_r1_double_backward_through_the_box_route(form):
    """conv_r1 -> pooled conv_r2 of a 16-px ResBlockDown under create_graph (the R1 regulariser): the forward of conv_r2 takes the box
    route, its backward under create_graph is ConvDgradFn on the folded weights as before - against the per-operator fp64 reference of
    tests/test_gpu_second_order.py."""
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    from tests.test_gpu_second_order import _ref_conv, _sn_state, compare
    N, C1, C2, H = 3, 16, 32, 16
    tag = "boxpool_r1"
    w1 = T(pf.normal(tag + "w1", (C2, C1, 3, 3)) / np.sqrt(C1 * 9))
    w2 = T(pf.normal(tag + "w2", (C2, C2, 3, 3)) / np.sqrt(C2 * 9))
    s1, u1, v1 = _sn_state(w1, tag + "1")
    s2, u2, v2 = _sn_state(w2, tag + "2")
    ins = {"x": T(pf.normal(tag + "x", (N, H, H, C1))), "w1": w1, "w2": w2, "b1": T(pf.normal(tag + "b1", (C2,))),
           "b2": T(pf.normal(tag + "b2", (C2,))), "s1": s1, "u1": u1, "v1": v1, "s2": s2, "u2": u2, "v2": v2}
    seen = {}

    def fwd_r(t):
        h = _ref_conv(t["x"], t["w1"], t["b1"], None, t["u1"], t["v1"], SLOPE, False)
        return (_ref_conv(h, t["w2"], t["b2"], None, t["u2"], t["v2"], SLOPE, True),)

    def fwd_p(t):
        h, act = ops.conv2d_post_act(t["x"], t["w1"], t["b1"], None, t["s1"], t["u1"], t["v1"], pre_slope=SLOPE, post_slope=SLOPE)
        with ops.count_flops() as c:
            y = ops.conv2d(h, t["w2"], t["b2"], None, t["s2"], t["u2"], t["v2"], 0, SLOPE, pool=True, x_act=act)
        seen.update(c)
        return (y,)

    compare(fwd_p, fwd_r, ins, ["x"], ["x", "w1", "w2", "b1", "b2"], tag, form)
    assert [cfg[7] for (kind, cfg) in seen if kind == "fwd"] == [2], seen
