"""GPU parity of the SECOND-ORDER operators, one node at a time: the R1 gradient penalty (training/utils.py:115-124) differentiates
the authenticator's input gradient once more, so every first-order backward on that path is itself an autograd operator whose adjoints
are other kernels of the same layer (ops.ConvDgradFn, AvgPool2BwdFn, MaxPoolLreluBwdFn, BgemmFn, SoftmaxDim1BwdFn, SetStatsBwdFn,
MulScalarFn; the differentiable fall-backs of ForkFn, ForkPoolFn, ConvForkPoolFn, ScaleAddFn under create_graph).

Every test does what training_utils.compute_grad2 does: the product operator on fp32 tensors, torch.autograd.grad(out, inputs, cot,
create_graph=True) inside ops.input_grad_only(), a scalar formed from the first-order gradients - a seeded random projection, or the
R1 form sum_b w_b * ops.sqsum_rows(g)[b] - and .backward().  The same program in fp64 plain torch is the reference.  Compared: the
first-order gradients (ConvDgradFn.forward is a different call path from ConvFn.backward) and the gradient of EVERY leaf - inputs,
weights, bias, gamma and the incoming cotangent (the adjoint w.r.t. the incoming gradient).  A leaf whose reference gradient is exactly
zero (a bias, an input behind a piecewise-linear map) must come back zero or None.

Convolutions run with a real spectral-norm state: u, v from two power iterations on W and sigma = u^T W v in fp64, so the
G / sigma - <G, W> / sigma^2 u v^T finish of the second-order weight gradient contributes (the first-order tests use u = v = 0).

Tolerances are relative L2 over the whole tensor.  The fp32 floor behind them is the SAME reference program run in fp32 torch on the
CPU against fp64 - measure_floor() below does that for any test of this file, without a GPU.  Measured: at most 1.5e-6 on the
convolution cases (the activated-storage pair, two dgrads in one chain), 4.5e-6 on the others (mean_std_cat with sets of 2 and 3),
and on the tuned-table shapes (N capped at 16) 1.7e-6 relative L2 and 4.3e-6 largest element.  The first-order bound of
tests/test_gpu_ops.py (TOL = 3e-5) is above 3x every floor, so it is kept, and the table shapes keep the pair of
tests/test_gpu_tuned_rows.py (3e-5 relative L2, 2e-4 largest element).  No per-tensor exemptions; the two places where the R1 form
itself is a cancellation (set statistics) are left out by construction (_set_leaves) and tested in the projection form.
"""
import contextlib
import ctypes
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import portable_fill as pf
from tests.helpers import T

pytestmark = pytest.mark.gpu

TOL = 3e-5          # relative L2, fp32 product vs fp64 reference (floors: module docstring)
TOL_MAX = 2e-4      # largest single-element error relative to the largest reference element (tuned-table shapes)
SLOPE = 0.2


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------------------------
# harness
# ------------------------------------------------------------------------------------------------------------------
class Fills:
    """Named fp64 tensors, made once and shared by the product and the reference run (cotangents, projections, row weights).
    `gen`: a torch.Generator on the GPU for the big tuned-table shapes; the portable fill (oracle/portable_fill.py) otherwise."""

    def __init__(self, tag, gen=None):
        self.tag, self.gen, self.cache = tag, gen, {}

    def __call__(self, name, shape, lo=-1.0, hi=1.0):
        key = (name, tuple(shape))
        if key not in self.cache:
            if self.gen is None:
                self.cache[key] = T(pf.uniform("%s/%s" % (self.tag, name), tuple(shape), lo, hi))
            else:
                self.cache[key] = torch.rand(tuple(shape), device=self.gen.device, generator=self.gen, dtype=torch.float64) * (hi - lo) + lo
        return self.cache[key]


def _prep(ins, dtype, device, product, leaves):
    t = {}
    for k, v in ins.items():
        if not torch.is_tensor(v):
            t[k] = v
            continue
        v = v.detach().to(device, dtype, copy=True)
        if product and v.dim() == 4 and k.startswith("w"):
            v = v.contiguous(memory_format=torch.channels_last)   # conv weights: logical [Cout,Cin,K,K], channels-last storage
        else:
            v = v.contiguous()
        if k in leaves:
            v.requires_grad_()
        t[k] = v
    return t


def run_double_backward(fwd, ins, xs, leaves, fills, form, dtype, device, product, pre=None):
    """fwd(t) -> tuple of outputs.  First-order gradients w.r.t. t[xs] with create_graph, a scalar of them (form "proj": random
    projection; "r1": sum_b w_b |g[b]|^2 through ops.sqsum_rows on the product side), backward.  pre: {leaf: fp64 G0} - an existing
    .grad the product ADDS into (the optimizer's flat bucket; weights in their channels-last memory order).
    Returns (outputs, first-order gradients, {leaf: .grad}, [cotangent .grad]) - detached."""
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    t = _prep(ins, dtype, device, product, set(leaves) | set(xs))
    if pre:
        for k, g0 in pre.items():
            t[k].grad = g0.to(device, dtype).contiguous(memory_format=torch.channels_last) if g0.dim() == 4 else g0.to(device, dtype).contiguous()
    outs = fwd(t)
    cots = [fills("cot%d" % i, o.shape).to(device, dtype, copy=True).requires_grad_() for i, o in enumerate(outs)]
    with (ops.input_grad_only() if product else contextlib.nullcontext()):
        gs = torch.autograd.grad(outs, [t[k] for k in xs], cots, create_graph=True)
    if form == "proj":
        L = sum((g * fills("proj_" + k, g.shape).to(device, dtype)).sum() for k, g in zip(xs, gs))
    else:
        L = 0
        for k, g in zip(xs, gs):
            g2 = g.reshape(g.shape[0], -1)
            sq = ops.sqsum_rows(g2) if product else g2.pow(2).sum(1)
            L = L + (sq * fills("roww_" + k, (g.shape[0],), 0.5, 1.5).to(device, dtype)).sum()
    L.backward()
    return ([o.detach() for o in outs], [g.detach() for g in gs], {k: t[k].grad for k in leaves}, [c.grad for c in cots])


def _err(got, ref):
    """(relative L2, largest element error / largest reference element); a reference that is exactly zero wants zero (None = zero)."""
    ref = ref.detach().double().cpu() if ref is not None else None
    got = got.detach().double().cpu() if got is not None else None
    if ref is None or float(ref.abs().max()) == 0.0:
        bad = 0.0 if got is None else float(got.abs().max())
        return (0.0, 0.0) if bad == 0.0 else (float("inf"), float("inf"))
    if got is None:
        return float("inf"), float("inf")
    d = got - ref
    return float(d.norm() / ref.norm()), float(d.abs().max() / ref.abs().max())


def compare(fwd_p, fwd_r, ins, xs, leaves, tag, form="proj", tol=TOL, tol_max=None, pre=None, fills=None, rdev="cpu",
            cmp_out=True, ins_p=None):
    """Product vs fp64 reference of one double backward; asserts every compared tensor.  ins_p: product-side replacements of some
    inputs under the same names (an input stored ACTIVATED: its gradient is the raw input's, compared with the reference's)."""
    fills = fills or Fills(tag)
    if _FLOOR:
        rdev = "cpu"
    o_r, g_r, l_r, c_r = run_double_backward(fwd_r, ins, xs, leaves, fills, form, torch.float64, rdev, False)
    if pre:
        # G0 of the size of the gradient added to it (fp32 rounding of the sum then stays far below the bound), rounded to fp32
        pre = {k: (g0 * (float(l_r[k].norm()) / float(g0.norm())) if l_r[k] is not None and float(l_r[k].norm()) > 0 else g0)
               .float().double() for k, g0 in pre.items()}
    if _FLOOR:   # measure_floor(): the same reference program in fp32 on the CPU in the product's place
        o_p, g_p, l_p, c_p = run_double_backward(fwd_r, ins, xs, leaves, fills, form, torch.float32, "cpu", False)
        pre = None
    else:
        o_p, g_p, l_p, c_p = run_double_backward(fwd_p, {**ins, **(ins_p or {})}, xs, leaves, fills, form, torch.float32, dev(), True, pre)
        torch.cuda.synchronize()
    rows = []
    if cmp_out:
        rows += [("out%d" % i, _err(a, b)) for i, (a, b) in enumerate(zip(o_p, o_r))]
    rows += [("d" + k, _err(a, b)) for k, a, b in zip(xs, g_p, g_r)]
    for k in leaves:
        got = l_p[k]
        if pre and k in pre and got is not None:
            got = got.double().cpu() - pre[k].cpu()     # G0 + the second-order gradient
        rows.append(("grad " + k, _err(got, l_r[k])))
    rows += [("grad cot%d" % i, _err(a, b)) for i, (a, b) in enumerate(zip(c_p, c_r))]
    if _FLOOR:
        _FLOOR[-1] += [(tag, form, nm, e) for nm, e in rows]
        return o_p, g_p, l_p, c_p
    bad = [(nm, e) for nm, e in rows if e[0] >= tol or (tol_max is not None and e[1] >= tol_max)]
    assert not bad, (tag, form, bad, rows)
    return o_p, g_p, l_p, c_p


def _sn_state(w, tag):
    """(sigma, u, v) as spectral norm holds them: u, v after two power iterations from seeded vectors, sigma = u^T W v (fp64;
    the reference differentiates sigma w.r.t. W with u, v constant).  v is indexed like W.reshape(Cout, -1) (logical order)."""
    Wm = w.reshape(w.shape[0], -1)
    g = torch.Generator(device=w.device).manual_seed(zlib.crc32(tag.encode()) & 0xFFFF)
    u = torch.randn(Wm.shape[0], dtype=torch.float64, device=w.device, generator=g)
    u = u / u.norm()
    for _ in range(2):
        v = Wm.t().mv(u)
        v = v / v.norm()
        u = Wm.mv(v)
        u = u / u.norm()
    return torch.dot(u, Wm.mv(v)).reshape(1), u, v


def _ref_conv(x, w, b, res, u, v, slope, pool):
    """fp64 reference of ops.conv2d on NHWC x: avgpool2?(conv(lrelu(x), W / sigma(W))) + b + res, sigma = u^T W v."""
    Cout, K = w.shape[0], w.shape[-1]
    wn = w / torch.dot(u, w.reshape(Cout, -1).mv(v)) if u is not None else w
    xa = F.leaky_relu(x, slope) if slope != 1.0 else x
    if x.dim() == 2:
        y = F.linear(xa, wn)
    else:
        y = F.conv2d(xa.permute(0, 3, 1, 2), wn, None, padding=(K - 1) // 2)
        if pool:
            y = F.avg_pool2d(y, 2)
        y = y.permute(0, 2, 3, 1)
    if b is not None:
        y = y + b
    if res is not None:
        y = y + res
    return y


def _plan(N, H, W, Cin, Cout, K, pool, kind):
    """gim_conv_launch_plan of the second-order launches' shape struct (ConvDgradFn.backward: no upsample, pre_slope = 1)."""
    from optimalstrategiesagainstgenerativeattacks_amd import _lib, ops
    sh = ops._shape(N, H, W, Cin, Cout, K, 0, 1.0, 1 if pool else 0, 1 if pool else 0, 0)
    out = (ctypes.c_int32 * 8)()
    _lib.check(_lib.load().gim_conv_launch_plan(ctypes.byref(sh), kind, ctypes.cast(out, ctypes.c_void_p)), "plan")
    return list(out)


_FLOOR = []


def measure_floor(test_fn, *args):
    """The fp32 floor behind a test's bounds: runs the test with compare() putting the SAME reference program in fp32 torch on the
    CPU where the product would run, and returns (largest relative L2, largest max-element error) over everything it compares.
    No GPU needed, e.g.  python -c "from tests.test_gpu_second_order import *; print(measure_floor(test_conv2d_double_backward,
    CONV_CASES[0], 'r1', False))"."""
    _FLOOR.append([])
    try:
        test_fn(*args)
    finally:
        rows = _FLOOR.pop()
    return max(e[0] for *_, e in rows), max(e[1] for *_, e in rows)


# ------------------------------------------------------------------------------------------------------------------
# convolutions
# ------------------------------------------------------------------------------------------------------------------
CONV_CASES = [
    # N, H, Cin, Cout, K, slope, pool, res, x_act, position-major (assert the skipped taps in the second-order forward)
    (2, 8, 16, 32, 3, 0.2, False, False, False, False),     # plain 3x3, LeakyReLU in front
    (2, 8, 16, 32, 3, 1.0, False, False, False, False),     # no activation: no mask in ConvDgradFn
    (2, 8, 16, 40, 3, 0.2, False, True, False, False),      # residual that requires grad; ragged Cout
    (3, 16, 32, 64, 3, 0.2, True, False, False, False),     # 3x3 + pool fold (stride-2, 4x4 taps)
    (3, 16, 32, 64, 1, 1.0, True, True, False, False),      # 1x1 + pool fold: the ResBlockDown skip
    (2, 16, 3, 64, 3, 0.2, False, False, False, False),     # image layer Cin = 3, W % 4 == 0: first-order dgrad gim_conv2d_dgrad_xfold
    (4, 2, 3, 32, 3, 0.2, False, False, False, False),      # Cin = 3, W = 2 (not a multiple of 4): gim_conv2d_dgrad_t
    (2, 16, 1, 32, 3, 0.2, False, False, False, False),     # Cin = 1
    (2, 16, 3, 64, 1, 1.0, True, False, False, False),      # the first block's 1x1 skip on the image
    (2, 8, 32, 48, 3, 0.2, False, False, True, False),      # x stored activated (x_act)
    (3, 8, 32, 64, 3, 0.2, True, False, True, False),       # x_act + pool fold
    (2, 8, 16, 20, 3, 0.2, True, False, False, False),      # ragged Cout + pool
    # >= 32 images on maps of <= 16 pixels: position-major rows, padding taps skipped (conv_igemm.hip PM_MAX_PIXELS / PM_MIN_IMAGES)
    (40, 4, 32, 48, 3, 0.2, False, True, False, True),      # 4x4
    (64, 2, 32, 64, 3, 0.2, False, False, False, True),     # 2x2
    (48, 1, 64, 64, 3, 1.0, False, False, False, True),     # 1x1 map, 3x3 kernel: only the centre tap
    (40, 8, 32, 32, 3, 0.2, True, True, False, True),       # 8x8 -> pooled 4x4
    (36, 4, 16, 48, 3, 0.2, True, False, True, True),       # 4x4 -> pooled 2x2, x_act
    (32, 2, 64, 64, 1, 1.0, True, False, False, False),     # 2x2 -> pooled 1x1, 1x1 skip (no padding taps to skip)
    # maps with H != W, given as (H, W)
    (2, (4, 16), 32, 48, 3, 0.2, False, False, False, False),    # patch-resident loop in the second-order forward
    (40, (2, 8), 32, 48, 3, 0.2, False, False, False, True),     # position-major rows
    (2, (16, 8), 32, 64, 3, 0.2, True, False, False, False),     # pool fold: 16x8 -> 8x4
]


def conv_case(N, H, Cin, Cout, K, slope, pool, use_res, x_act, pm):
    tag = "so_conv%s" % ((N, H, Cin, Cout, K, slope, pool, use_res, x_act),)
    H, W = (H, H) if isinstance(H, int) else H       # one side of a square map, or (H, W)
    x = T(pf.normal(tag + "x", (N, H, W, Cin)))
    w = T(pf.normal(tag + "w", (Cout, Cin, K, K)) / np.sqrt(Cin * K * K))
    b = T(pf.normal(tag + "b", (Cout,)))
    sigma, u, v = _sn_state(w, tag)
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    ins = {"x": x, "w": w, "b": b, "sigma": sigma, "u": u, "v": v}
    if use_res:
        ins["res"] = T(pf.normal(tag + "r", (N, Ho, Wo, Cout)))

    def fwd_r(t):
        return (_ref_conv(t["x"], t["w"], t["b"], t.get("res"), t["u"], t["v"], slope, pool),)

    xs = ["x"] + (["res"] if use_res else [])
    return fwd_r, ins, xs, ["x", "w", "b"], tag


@pytest.mark.parametrize("queued", [False, True], ids=["own", "queued"])
@pytest.mark.parametrize("form", ["proj", "r1"])
@pytest.mark.parametrize("case", CONV_CASES, ids=[str(c) for c in CONV_CASES])
def test_conv2d_double_backward(case, form, queued):
    """ops.conv2d through ConvDgradFn: first-order dx (+ dres), and the second-order gradients w.r.t. x (zero: the mask is piecewise
    constant), W (the wgrad kernel with the masked cotangent as the layer input + the spectral-norm finish), the bias (zero) and the
    incoming cotangent (the forward kernel on the masked cotangent).  queued: w.grad / b.grad pre-exist as dense buffers holding G0 in
    the weights' memory order - the FusedAdam bucket of a training step - so the weight gradient is ADDED there by the batched finish.
    x_act: the product reads x stored activated (lrelu(x)) and hands back the gradient w.r.t. the raw x."""
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    N, H, Cin, Cout, K, slope, pool, use_res, x_act, pm = case
    fwd_r, ins, xs, leaves, tag = conv_case(*case)

    def fwd_p(t):
        return (ops.conv2d(t["x"], t["w"], t["b"], t.get("res"), t["sigma"], t["u"], t["v"], 0, slope, pool=pool, x_act=x_act),)

    compare(fwd_p, fwd_r, ins, xs, leaves, tag, form, pre=_g0(ins, tag) if queued else None,
            ins_p={"x": F.leaky_relu(ins["x"], slope)} if x_act else None)
    assert not ops.wgrad_queue.jobs
    if pm:
        # the second-order forward launch (the forward kernel on the masked cotangent: bias None, pre_slope 1) runs position-major
        # rows and skips the padding taps (launch plan out[7] bits 8 and up: the skipped share of the K steps)
        assert _plan(N, *ins["x"].shape[1:3], Cin, Cout, K, pool, 0)[7] >> 8 > 0, ("second-order forward is not position-major", case)


def _g0(ins, tag):
    """Known non-zero contents of the pre-existing .grad buffers of w and b (queued path)."""
    return {"w": T(pf.uniform(tag + "g0w", tuple(ins["w"].shape))), "b": T(pf.uniform(tag + "g0b", tuple(ins["b"].shape)))}


FORKPOOL_CASES = [
    # N, H, Cin, Cout, K, x_act (x stored activated: the pool inverts the LeakyReLU, in_slope = 0.2)
    (2, 8, 32, 48, 3, True),
    (2, 8, 32, 48, 3, False),
    (40, 4, 32, 64, 3, True),       # position-major rows
    (2, 16, 3, 64, 3, False),       # image channels: x-fold dgrad
]


@pytest.mark.parametrize("form", ["proj", "r1"])
@pytest.mark.parametrize("case", FORKPOOL_CASES, ids=[str(c) for c in FORKPOOL_CASES])
def test_conv2d_forkpool_double_backward(case, form):
    """ops.conv2d_forkpool (ConvForkPoolFn: the conv and the pooled skip reader of a ResBlockDown input as ONE node): under
    create_graph its backward is the unfused sum ConvDgradFn + AvgPool2BwdFn; two outputs, two cotangents."""
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    N, H, Cin, Cout, K, x_act = case
    tag = "so_cfp%s" % (case,)
    x = T(pf.normal(tag + "x", (N, H, H, Cin)))
    w = T(pf.normal(tag + "w", (Cout, Cin, K, K)) / np.sqrt(Cin * K * K))
    sigma, u, v = _sn_state(w, tag)
    ins = {"x": x, "w": w, "b": T(pf.normal(tag + "b", (Cout,))), "sigma": sigma, "u": u, "v": v}

    def fwd_r(t):
        return (_ref_conv(t["x"], t["w"], t["b"], None, t["u"], t["v"], SLOPE, False),
                F.avg_pool2d(t["x"].permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1))

    def fwd_p(t):
        y, act, pooled = ops.conv2d_forkpool(t["x"], t["w"], t["b"], t["sigma"], t["u"], t["v"], SLOPE, None, 1.0, x_act,
                                             SLOPE if x_act else 1.0)
        assert not act
        return y, pooled

    compare(fwd_p, fwd_r, ins, ["x"], ["x", "w", "b"], tag, form, ins_p={"x": F.leaky_relu(x, SLOPE)} if x_act else None)


@pytest.mark.parametrize("N,C1,C2,H,expect_act", [(6, 16, 64, 32, True), (2, 64, 64, 4, False), (40, 32, 32, 4, False)])
def test_conv_pair_with_activated_storage_double_backward(N, C1, C2, H, expect_act):
    """conv_r1 (ops.conv2d_post_act: output stored activated where the launch allows) -> pooled conv_r2 with x_act, the ResBlockDown
    pair, through the R1 form: two ConvDgradFn in one chain (the sqsum's gradient 2 w_b dx is itself a product of both dgrads)."""
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    tag = "so_pair%d_%d_%d_%d" % (N, C1, C2, H)
    w1 = T(pf.normal(tag + "w1", (C2, C1, 3, 3)) / np.sqrt(C1 * 9))
    w2 = T(pf.normal(tag + "w2", (C2, C2, 3, 3)) / np.sqrt(C2 * 9))
    s1, u1, v1 = _sn_state(w1, tag + "1")
    s2, u2, v2 = _sn_state(w2, tag + "2")
    ins = {"x": T(pf.normal(tag + "x", (N, H, H, C1))), "w1": w1, "w2": w2, "b1": T(pf.normal(tag + "b1", (C2,))),
           "b2": T(pf.normal(tag + "b2", (C2,))), "s1": s1, "u1": u1, "v1": v1, "s2": s2, "u2": u2, "v2": v2}

    def fwd_r(t):
        h = _ref_conv(t["x"], t["w1"], t["b1"], None, t["u1"], t["v1"], SLOPE, False)
        return (_ref_conv(h, t["w2"], t["b2"], None, t["u2"], t["v2"], SLOPE, True),)

    def fwd_p(t):
        h, act = ops.conv2d_post_act(t["x"], t["w1"], t["b1"], None, t["s1"], t["u1"], t["v1"], pre_slope=SLOPE, post_slope=SLOPE)
        assert act == expect_act, "which regime this shape was meant to exercise"
        return (ops.conv2d(h, t["w2"], t["b2"], None, t["s2"], t["u2"], t["v2"], 0, SLOPE, pool=True, x_act=act),)

    for form in ("proj", "r1"):
        compare(fwd_p, fwd_r, ins, ["x"], ["x", "w1", "w2", "b1", "b2"], tag, form)


@pytest.mark.parametrize("rows,din,dout,slope", [(5, 6, 10, 0.2), (16, 3, 33, 1.0), (80, 512, 130, 0.2), (40, 1536, 64, 1.0)])
def test_linear_double_backward(rows, din, dout, slope):
    """ops.linear (2-D ConvFn, no spectral norm): Cin <= 8 and wide Cin, ragged outputs."""
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    tag = "so_lin%d_%d_%d" % (rows, din, dout)
    ins = {"x": T(pf.normal(tag + "x", (rows, din))), "w": T(pf.normal(tag + "w", (dout, din)) / np.sqrt(din)),
           "b": T(pf.normal(tag + "b", (dout,)))}

    def fwd_r(t):
        return (_ref_conv(t["x"], t["w"], t["b"], None, None, None, slope, False),)

    def fwd_p(t):
        return (ops.linear(t["x"], t["w"], t["b"], slope),)

    for form in ("proj", "r1"):
        compare(fwd_p, fwd_r, ins, ["x"], ["x", "w", "b"], tag, form)
        compare(fwd_p, fwd_r, ins, ["x"], ["x", "w", "b"], tag, form, pre=_g0(ins, tag))


# ------------------------------------------------------------------------------------------------------------------
# every shape of the tuned launch table (csrc/conv_tune_table.inc) that the second order can reach (no upsampling)
# ------------------------------------------------------------------------------------------------------------------
def _tuned_shapes():
    from tests.test_gpu_tuned_rows import SHAPES
    return [c for c in SHAPES if c[6] == 0]


TUNED = _tuned_shapes()


@pytest.mark.parametrize("cfg", TUNED, ids=[",".join(str(c) for c in s) for s in TUNED])
def test_tuned_shape_double_backward_vs_fp64(cfg):
    """Each (N, H, W, Cin, Cout, K, 0, slope, pool, fold) of the table in the R1 form, as a training step runs it: spectral-norm
    state, pre-existing .grad buffers in the weights' memory order (the queued arena and the batched finish ADD the R1 weight
    gradient to G0).  The second-order forward launch (bias None, pre_slope 1) must resolve to the same table row as the layer's
    first-order forward (DESIGN.md "Second order").  Elementwise check: relative L2 and largest-element error."""
    from tests.test_gpu_tuned_rows import ROWS, _ref_device
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    N, H, W, Cin, Cout, K, ups, slope, pool, fold = cfg
    if any(r[0] == 0 and r[9] == cfg for r in ROWS):
        assert _plan(N, H, W, Cin, Cout, K, pool, 0)[0] == 1, ("second-order forward misses the table row", cfg)
    d = torch.device("cpu") if _FLOOR else dev()
    g = torch.Generator(device=d).manual_seed(hash(cfg) & 0xFFFF)
    x = torch.randn(N, H, W, Cin, device=d, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, Cin, K, K, device=d, generator=g, dtype=torch.float64) / (Cin * K * K) ** 0.5
    b = torch.randn(Cout, device=d, generator=g, dtype=torch.float64)
    sigma, u, v = _sn_state(w, "tuned%s" % (cfg,))
    ins = {"x": x, "w": w, "b": b, "sigma": sigma, "u": u, "v": v}
    pre = {"w": torch.rand(w.shape, device=d, generator=g, dtype=torch.float64) - 0.5,
           "b": torch.rand(b.shape, device=d, generator=g, dtype=torch.float64) - 0.5}
    fills = Fills("tuned", gen=g)

    def fwd_r(t):
        return (_ref_conv(t["x"], t["w"], t["b"], None, t["u"], t["v"], slope, pool),)

    def fwd_p(t):
        return (ops.conv2d(t["x"], t["w"], t["b"], None, t["sigma"], t["u"], t["v"], 0, slope, pool=bool(pool)),)

    compare(fwd_p, fwd_r, ins, ["x"], ["x", "w", "b"], "tuned%s" % (cfg,), "r1", tol_max=TOL_MAX, pre=pre, fills=fills,
            rdev=_ref_device())
    assert not ops.wgrad_queue.jobs


# ------------------------------------------------------------------------------------------------------------------
# determinism
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(4, 8, 32, 64, 3, 0.2, False), (4, 16, 32, 64, 3, 0.2, True), (40, 4, 32, 48, 3, 0.2, False),
                                  (16, 8, 256, 512, 3, 0.2, True)])
def test_double_backward_bit_reproducible_in_deterministic_mode(case):
    """Under ops.set_deterministic(True) two runs of the same double backward give identical first-order and second-order
    gradients (no split-K atomics in the forward / dgrad launches, weight gradients as slabs added in a fixed order)."""
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    N, H, Cin, Cout, K, slope, pool = case
    tag = "so_det%s" % (case,)
    x = T(pf.normal(tag + "x", (N, H, H, Cin)))
    w = T(pf.normal(tag + "w", (Cout, Cin, K, K)) / np.sqrt(Cin * K * K))
    sigma, u, v = _sn_state(w, tag)
    ins = {"x": x, "w": w, "b": T(pf.normal(tag + "b", (Cout,))), "sigma": sigma, "u": u, "v": v}
    fills = Fills(tag)

    def fwd_p(t):
        return (ops.conv2d(t["x"], t["w"], t["b"], None, t["sigma"], t["u"], t["v"], 0, slope, pool=pool),)

    prev = ops.set_deterministic(True)
    try:
        runs = [run_double_backward(fwd_p, ins, ["x"], ["x", "w"], fills, "r1", torch.float32, dev(), True) for _ in range(2)]
    finally:
        ops.set_deterministic(prev)
    (_, g1, l1, c1), (_, g2, l2, c2) = runs
    assert torch.equal(g1[0], g2[0]) and torch.equal(l1["w"], l2["w"]) and torch.equal(c1[0], c2[0])
    assert l1["x"] is None and l2["x"] is None


# ------------------------------------------------------------------------------------------------------------------
# everything else on the R1 path
# ------------------------------------------------------------------------------------------------------------------
def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


@pytest.mark.parametrize("in_slope", [1.0, SLOPE])
def test_avg_pool2_double_backward(in_slope):
    """AvgPool2Fn -> AvgPool2BwdFn -> AvgPool2Fn.  in_slope != 1: x stored activated, gradient w.r.t. the raw x."""
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    tag = "so_pool%g" % in_slope
    x = T(pf.normal(tag + "x", (3, 8, 6, 70)))
    for form in ("proj", "r1"):
        compare(lambda t: (ops.avg_pool2(t["x"], in_slope),), lambda t: (_nhwc(F.avg_pool2d(_nchw(t["x"]), 2)),), {"x": x}, ["x"], ["x"],
                tag, form, ins_p={"x": F.leaky_relu(x, in_slope)} if in_slope != 1.0 else None)


@pytest.mark.parametrize("n", [2, 3, 5])
def test_fork_double_backward(n):
    """ForkFn with n consumers: under create_graph the gradient sum is built from differentiable additions."""
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    tag = "so_fork%d" % n
    x = T(pf.normal(tag + "x", (4, 5, 5, 24)))
    cs = [float(i + 1) * 0.3 for i in range(n)]

    def consumers(xs_):
        return tuple(xi * xi * c if i % 2 == 0 else xi * c for i, (xi, c) in enumerate(zip(xs_, cs)))

    for form in ("proj", "r1"):
        compare(lambda t: consumers(ops.fork(t["x"], n)), lambda t: consumers((t["x"],) * n), {"x": x}, ["x"], ["x"], tag, form)


@pytest.mark.parametrize("in_slope", [1.0, SLOPE])
def test_fork_pool_double_backward(in_slope):
    """ForkPoolFn (alias for the conv path, avgpool2 for the skip path): differentiable sum under create_graph."""
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    tag = "so_forkpool%g" % in_slope
    x = T(pf.normal(tag + "x", (3, 8, 8, 40)))

    def fwd_p(t):
        a, p = ops.fork_pool(t["x"], in_slope)
        return a * 0.7, p       # (the alias's consumer hands back the gradient w.r.t. the raw x, as a conv with x_act does)

    def fwd_r(t):
        return t["x"] * 0.7, _nhwc(F.avg_pool2d(_nchw(t["x"]), 2))

    for form in ("proj", "r1"):
        compare(fwd_p, fwd_r, {"x": x}, ["x"], ["x"], tag, form, cmp_out=in_slope == 1.0,
                ins_p={"x": F.leaky_relu(x, in_slope)} if in_slope != 1.0 else None)


@pytest.mark.parametrize("HW", [1, 4, 8])
def test_maxpool_lrelu_double_backward(HW):
    """MaxPoolLreluFn -> MaxPoolLreluBwdFn -> gim_maxpool_gather on H*W = 1, 16, 64 pixels; a third of the channels have an all-negative
    set (the slope branch of lrelu' at the maximum); values distinct (no arg-max ties)."""
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    tag = "so_maxpool%d" % HW
    N, C = 5, 67
    x = T(pf.normal(tag + "x", (N, HW, HW, C)))
    x[:, :, :, ::3] = -x[:, :, :, ::3].abs() - 0.1
    assert (x.amax(dim=(1, 2))[:, ::3] < 0).all()
    assert all(len(set(x[n, :, :, c].flatten().tolist())) == HW * HW for n in range(N) for c in range(C))

    def fwd_r(t):
        return (F.leaky_relu(F.adaptive_max_pool2d(_nchw(t["x"]), (1, 1)).reshape(N, C), SLOPE),)

    for form in ("proj", "r1"):
        compare(lambda t: (ops.maxpool_lrelu(t["x"]),), fwd_r, {"x": x}, ["x"], ["x"], tag, form)


@pytest.mark.parametrize("gamma", [0.0, 0.7])
def test_scale_add_double_backward(gamma):
    """ScaleAddFn (SelfAttention's gamma * attention + x) -> MulScalarFn under create_graph.  gamma = 0 is the module's initial value:
    the R1 gradient w.r.t. gamma is <projection, cotangent> there and must not vanish."""
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    tag = "so_scaleadd%g" % gamma
    ins = {"a": T(pf.normal(tag + "a", (3, 4, 4, 32))), "x": T(pf.normal(tag + "x", (3, 4, 4, 32))), "gamma": torch.tensor([gamma], dtype=torch.float64)}
    for form in ("proj", "r1"):
        _, _, l_p, _ = compare(lambda t: (ops.scale_add(t["a"], t["x"], t["gamma"]),), lambda t: (t["gamma"] * t["a"] + t["x"],), ins,
                               ["a", "x"], ["a", "x", "gamma"], tag, form)
        if form == "proj":   # (the R1 form of this isolated node has d/dgamma = 2 gamma |cot|^2: zero at gamma = 0)
            assert l_p["gamma"] is not None and float(l_p["gamma"].abs()) > 0


@pytest.mark.parametrize("tA,tB", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_bgemm_double_backward(tA, tB):
    """BgemmFn, every transpose combination, odd sizes: its backward is BgemmFn again (bilinear)."""
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    nb, M, N, K = 3, 37, 29, 19
    tag = "so_bgemm%d%d" % (tA, tB)
    ins = {"A": T(pf.normal(tag + "A", (nb, K, M) if tA else (nb, M, K))), "B": T(pf.normal(tag + "B", (nb, N, K) if tB else (nb, K, N)))}

    def fwd_r(t):
        return (torch.matmul(t["A"].transpose(1, 2) if tA else t["A"], t["B"].transpose(1, 2) if tB else t["B"]),)

    for form in ("proj", "r1"):
        compare(lambda t: (ops.BgemmFn.apply(t["A"], t["B"], tA, tB),), fwd_r, ins, ["A", "B"], ["A", "B"], tag, form)


@pytest.mark.parametrize("R,C", [(37, 70), (64, 64), (200, 129), (256, 16), (300, 65)])
def test_softmax_dim1_double_backward(R, C):
    """SoftmaxDim1Fn -> SoftmaxDim1BwdFn (gim_softmax_dim1_bwd for d/d dP, gim_softmax_dim1_bwd_dp for d/dP) with R <= 64, 65..256 and
    > 256 rows (the <16> / <64> register kernels and the generic one) and column counts that are not multiples of 64."""
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    tag = "so_softmax%d_%d" % (R, C)
    S = T(pf.normal(tag + "S", (2, R, C))) * 2.0
    for form in ("proj", "r1"):
        compare(lambda t: (ops.SoftmaxDim1Fn.apply(t["S"]),), lambda t: (torch.softmax(t["S"], dim=1),), {"S": S}, ["S"], ["S"], tag, form)


@pytest.mark.parametrize("T_,K,Ch", [(256, 16, 24), (64, 8, 16), (300, 16, 20)])
def test_attn_core_double_backward(T_, K, Ch):
    """ops.attn_core: the fused AttnProbFn (T = 256, K = 16, the benchmark networks' attention) and the unfused BgemmFn + SoftmaxDim1Fn
    form; out = softmax_dim1(f g^T)^T h."""
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    tag = "so_attn%d_%d_%d" % (T_, K, Ch)
    ins = {"f": T(pf.normal(tag + "f", (2, T_, K))) * 0.5, "g": T(pf.normal(tag + "g", (2, T_, K))) * 0.5, "h": T(pf.normal(tag + "h", (2, T_, Ch)))}
    assert ops.AttnProbFn.supported(ins["f"], ins["g"]) == (T_ == 256 and K == 16)

    def fwd_r(t):
        A = torch.softmax(torch.matmul(t["f"], t["g"].transpose(1, 2)), dim=1)
        return (torch.matmul(A.transpose(1, 2), t["h"]),)

    for form in ("proj", "r1"):
        compare(lambda t: (ops.attn_core(t["f"], t["g"], t["h"]),), fwd_r, ins, ["f", "g", "h"], ["f", "g", "h"], tag, form)


def _custom_std(x):
    """models/model_blocks.py:41-48 (oracle/gim_oracle.py custom_std): a set of one has std 0, a constant."""
    if x.shape[1] > 1:
        return torch.sqrt(x.var(1) + 1e-8)
    return torch.zeros((x.shape[0],) + tuple(x.shape[2:]), dtype=x.dtype, device=x.device)


SET_SIZES = [(1, 10), (5, 2), (10, 1), (2, 5)]


def _set_leaves(form, sets):
    """Leaves whose second-order gradient is compared; sets = {name: (set size, has a custom_std slot)}.  Left out, because the
    reference gradient is a pure cancellation there (fp32 torch is 3 % - 8x of its own size off, and so would any correct kernel be):
    - in the R1 form, every set input: with dx_j = dm / t + ds (x_j - m) / ((t - 1) sd) the squared norm sum_j |dx_j|^2 =
      |dm|^2 / t + |ds|^2 var / ((t - 1) (var + 1e-8)) does not depend on x;
    - a set of TWO with a std slot: the std of two points is |x_1 - x_2| / sqrt(2) (+ the 1e-8), whose gradient is piecewise
      constant, so the x gradient is the 1e-8 alone.
    The projection form tests gim_set_stats_bwd_bwd's gx on every other input; the R1 form still checks the first-order gradients and
    the adjoint w.r.t. the cotangent (its g_dmean / g_dstd)."""
    return [nm for nm, (t, has_std) in sets.items() if form == "proj" and not (has_std and t == 2)]


@pytest.mark.parametrize("n,k", SET_SIZES)
def test_head_cat_double_backward(n, k):
    """ops.head_cat (the authenticator head's set statistics) -> SetStatsBwdFn -> gim_set_stats_bwd_bwd, set sizes 1, 2, 5, 10; widths
    not multiples of 256."""
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    B, Ds, De, Df = 3, 300, 270, 37
    tag = "so_head%d_%d" % (n, k)
    shapes = {"ts": (B, n, Ds), "te": (B, n, De), "ss": (B, k, Ds), "se": (B, k, De), "ft": (B, n, Df), "fs": (B, k, Df)}
    ins = {nm: T(pf.normal(tag + nm, s)) for nm, s in shapes.items()}
    names = list(shapes)

    def fwd_r(t):
        return (torch.cat((t["ts"].mean(1), t["ss"].mean(1), t["te"].mean(1), _custom_std(t["te"]), t["ft"].mean(1),
                           t["se"].mean(1), _custom_std(t["se"]), t["fs"].mean(1)), dim=-1),)

    for form in ("proj", "r1"):
        compare(lambda t: (ops.head_cat(*[t[nm] for nm in names]),), fwd_r, ins, names, _set_leaves(form, {nm: (n if nm in ("ts", "te", "ft") else k, nm in ("te", "se")) for nm in names}), tag, form)


@pytest.mark.parametrize("t_", [1, 2, 5, 10])
def test_stat_cat_and_mean_std_cat_double_backward(t_):
    """ops.stat_cat ([mean, custom_std](x), mean(fc)) and ops.mean_std_cat (two sets of sizes t and t + 1) -> SetStatsBwdFn."""
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    B, D, Df = 4, 130, 300
    tag = "so_stat%d" % t_
    ins = {"x": T(pf.normal(tag + "x", (B, t_, D))), "fc": T(pf.normal(tag + "fc", (B, t_, Df)))}
    for form in ("proj", "r1"):
        compare(lambda t: (ops.stat_cat(t["x"], t["fc"]),), lambda t: (torch.cat((t["x"].mean(1), _custom_std(t["x"]), t["fc"].mean(1)), -1),),
                ins, ["x", "fc"], _set_leaves(form, {"x": (t_, True), "fc": (t_, False)}), tag, form)
    ins2 = {"a": T(pf.normal(tag + "a", (B, t_, D))), "b": T(pf.normal(tag + "b", (B, t_ + 1, D)))}

    def fwd_r2(t):
        return (torch.cat((t["a"].mean(1), _custom_std(t["a"]), t["b"].mean(1), _custom_std(t["b"])), -1),)

    for form in ("proj", "r1"):
        compare(lambda t: (ops.mean_std_cat(t["a"], t["b"]),), fwd_r2, ins2, ["a", "b"], _set_leaves(form, {"a": (t_, True), "b": (t_ + 1, True)}), tag + "ms", form)


@pytest.mark.parametrize("B,L", [(1, 5), (16, 3 * 64 * 64), (7, 1000)])
def test_sqsum_rows(B, L):
    """ops.sqsum_rows (compute_grad2's per-episode squared norm) and its backward, against fp64."""
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    tag = "so_sqsum%d_%d" % (B, L)
    x = T(pf.normal(tag + "x", (B, L)))
    r = T(pf.uniform(tag + "r", (B,)))
    xr = x.clone().requires_grad_()
    yr = xr.pow(2).sum(1)
    (yr * r).sum().backward()
    xg = x.float().to(dev()).requires_grad_()
    yg = ops.sqsum_rows(xg)
    (yg * r.float().to(dev())).sum().backward()
    assert _err(yg, yr)[0] < TOL and _err(xg.grad, xr.grad)[0] < TOL


@pytest.mark.parametrize("C", [1, 3])
def test_layout_double_backward(C):
    """ops.to_nhwc / ops.to_nchw (each the other's backward; C = 1 is a view)."""
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    tag = "so_layout%d" % C
    x = T(pf.normal(tag + "x", (3, C, 8, 6)))
    y = T(pf.normal(tag + "y", (3, 8, 6, C)))
    for form in ("proj", "r1"):
        compare(lambda t: (ops.to_nhwc(t["x"]) * 1.5,), lambda t: (t["x"].permute(0, 2, 3, 1) * 1.5,), {"x": x}, ["x"], ["x"], tag, form)
        compare(lambda t: (ops.to_nchw(t["y"]) * 1.5,), lambda t: (t["y"].permute(0, 3, 1, 2) * 1.5,), {"y": y}, ["y"], ["y"], tag, form)


# ------------------------------------------------------------------------------------------------------------------
# contract pins: what the second order refuses
# ------------------------------------------------------------------------------------------------------------------
def _small_conv(ups=0, res_ups=False):
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    d = dev()
    x = torch.randn(2, 4, 4, 16, device=d).requires_grad_()
    w = (torch.randn(32, 16, 3, 3, device=d) / 12).contiguous(memory_format=torch.channels_last).requires_grad_()
    res = torch.randn(2, 4, 4, 32, device=d) if res_ups else None
    y = ops.conv2d(x, w, None, res, None, None, None, ups, SLOPE, res_ups=res_ups)
    return x, w, y


def test_create_graph_outside_input_grad_only_is_refused():
    x, _, y = _small_conv()
    with pytest.raises(NotImplementedError):
        torch.autograd.grad(y, x, torch.ones_like(y), create_graph=True)


def test_third_order_is_refused():
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    x, w, y = _small_conv()
    with ops.input_grad_only():
        (gx,) = torch.autograd.grad(y, x, torch.ones_like(y), create_graph=True)
        with pytest.raises(NotImplementedError):
            torch.autograd.grad(gx, w, torch.ones_like(gx), create_graph=True)
    xs = torch.randn(3, 10, device=dev()).requires_grad_()
    s = ops.sqsum_rows(xs)
    with ops.input_grad_only():
        with pytest.raises(NotImplementedError):
            torch.autograd.grad(s, xs, torch.ones_like(s), create_graph=True)


@pytest.mark.parametrize("ups,res_ups", [(1, False), (0, True)])
def test_second_order_of_an_upsampling_conv_is_refused(ups, res_ups):
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    x, _, y = _small_conv(ups, res_ups)
    with ops.input_grad_only():
        with pytest.raises(NotImplementedError):
            torch.autograd.grad(y, x, torch.ones_like(y), create_graph=True)
