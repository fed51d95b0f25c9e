"""GPU parity on maps with H != W.  The convolution C ABI takes H and W as independent powers of two and every kernel carries logH and
logW, but the product's workloads - and so every other parity case of the implicit-GEMM kernels - are square: a kernel that swaps H and W
in a patch, halo, permutation or row-walk computation passes them all.  Here every kernel family runs on rectangles, both orientations,
against fp64 F.conv2d: the rows of tests/helpers.py RECT_CASES through ops.conv2d (tests/test_host.py asserts on the CPU that each row
reaches the family it names), the weight-gradient, x-fold and inference entry points directly, the fp16 twins, and the pointwise
operators that take H and W.  (The second-order cases are in tests/test_gpu_second_order.py.)  No tolerance is new: TOL of
test_gpu_ops.py, 1e-5 of its direct weight-gradient tests, TOL / TOL_ROUND of test_gpu_fp16.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import portable_fill as pf
from tests.helpers import (RECT_CASES, RECT_IDS, RECT_WGRAD_ROW_CASES, RectCase, T, assert_rect_wgrad_row_plan, conv_fwd_bwd, epi_plan, rect_plan,
                           rect_wgrad_row_shape, relerr)
from tests.test_gpu_fp16 import TOL_ROUND, fp16_path, r16  # noqa: F401  (fp16_path: a fixture)

pytestmark = pytest.mark.gpu

TOL = 3e-5
TOL_WGRAD = 1e-5
ULP2 = 2.0 ** -22     # the copy kernels: one fp32 addition and one multiplication per element, 2^-24 each at the most, on fp32 inputs


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def nhwc(x):  # NCHW cpu f64 -> NHWC cuda f32
    return x.detach().permute(0, 2, 3, 1).contiguous().float().to(dev())


def nchw(y):  # NHWC cuda -> NCHW cpu f64
    return y.detach().permute(0, 3, 1, 2).double().cpu()


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("queued", [False, True], ids=["own", "queued"])
@pytest.mark.parametrize("case", RECT_CASES, ids=RECT_IDS)
def test_rect_conv2d_fwd_bwd(case, queued):
    """One row of RECT_CASES: the plan it records, then y, dx, dw, db (and dres) against fp64 autograd.  queued: weight and bias own
    .grad buffers, as in a training step - the weight gradient goes through gim_conv2d_wgrad_acc (the image layers: the row-padded slot of
    gim_conv2d_wgrad_rows_acc and fold code 3 of the batched finish) and is added there."""
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    assert rect_plan(ops, case) == case.plan, case.name
    N, H, W, Cin, Cout, K, ups, pool, slope, res = case.geom
    print("rect %s %s plan %s" % (case.name, case.geom, case.plan))
    conv_fwd_bwd(ops, "rect_" + case.name, N, (H, W), Cin, Cout, K, ups, bool(pool), slope, res, 1.7, TOL, 0.25 if queued else None, case.tune,
                 keep_ref=True)


@pytest.mark.parametrize("case", RECT_WGRAD_ROW_CASES, ids=[str(c) for c in RECT_WGRAD_ROW_CASES])
def test_rect_wgrad_row_resident_3x3(case):
    """gim_conv2d_wgrad_acc with tile code 20000 on rectangles: rows of min(W, 16) pixels, 16 / min(W, 16) image rows per step - and the
    two maps of fewer than 4 columns, which the plan must hand to the MFMA kernel.  Adds into a pre-filled slot; fp64 autograd of F.conv2d."""
    from optimalstrategiesagainstgenerativeattacks_amd import _lib
    lib = _lib.load()
    N, H, W, Cin, Cout, _ = case
    assert_rect_wgrad_row_plan(case)
    g = torch.Generator(device="cuda").manual_seed(37)
    x = torch.randn(N, H, W, Cin, device=dev(), generator=g)
    dy = torch.randn(N, H, W, Cout, device=dev(), generator=g)
    sh = rect_wgrad_row_shape(case)
    pre_w = torch.randn(Cout * 9 * Cin, device=dev(), generator=g)
    pre_b = torch.randn(Cout, device=dev(), generator=g)
    acc, bacc = pre_w.clone(), pre_b.clone()
    _lib.check(lib.gim_conv2d_wgrad_acc(dy.data_ptr(), x.data_ptr(), acc.data_ptr(), bacc.data_ptr(), sh, _stream()), "wgrad_acc")
    wr = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64, device=dev(), requires_grad=True)
    br = torch.zeros(Cout, dtype=torch.float64, device=dev(), requires_grad=True)
    yr = F.conv2d(F.leaky_relu(x.double().permute(0, 3, 1, 2), 0.2), wr, br, padding=1)
    (yr * dy.double().permute(0, 3, 1, 2)).sum().backward()
    got = (acc - pre_w).view(Cout, 3, 3, Cin).permute(0, 3, 1, 2)
    ew, eb = relerr(got.double(), wr.grad), relerr((bacc - pre_b).double(), br.grad)
    print("rect wgrad_row %s: dw %.2e db %.2e" % (case, ew, eb))
    assert ew < TOL_WGRAD and eb < TOL_WGRAD


@pytest.mark.parametrize("N,H,W,Cin,Cout", [(16, 8, 32, 3, 64), (16, 32, 8, 64, 3)])
def test_rect_wgrad_1x1_narrow_side(N, H, W, Cin, Cout):
    """The outer-product kernel of the 1x1 image skip convs (plan: no tile) on rectangles, adding into a pre-filled slot."""
    from optimalstrategiesagainstgenerativeattacks_amd import _lib
    lib = _lib.load()
    sh = _lib.GimConvShape(N, H, W, Cin, Cout, 1, 0, 0.2)
    plan = epi_plan(sh, 3)
    assert plan[1:3] == [0, 0] and plan[7] == 0, plan
    g = torch.Generator(device="cuda").manual_seed(13)
    x = torch.randn(N, H, W, Cin, device=dev(), generator=g)
    dy = torch.randn(N, H, W, Cout, device=dev(), generator=g)
    pre_w = torch.randn(Cout * Cin, device=dev(), generator=g)
    pre_b = torch.randn(Cout, device=dev(), generator=g)
    acc, bacc = pre_w.clone(), pre_b.clone()
    _lib.check(lib.gim_conv2d_wgrad_acc(dy.data_ptr(), x.data_ptr(), acc.data_ptr(), bacc.data_ptr(), sh, _stream()), "wgrad_acc")
    ref = torch.einsum("nhwo,nhwc->oc", dy.double(), F.leaky_relu(x.double(), 0.2))
    ew = relerr(acc.view(Cout, Cin).double() - pre_w.view(Cout, Cin).double(), ref)
    eb = relerr(bacc.double() - pre_b.double(), dy.double().sum((0, 1, 2)))
    print("rect wgrad_1x1 %s: dw %.2e db %.2e" % ((N, H, W, Cin, Cout), ew, eb))
    assert ew < TOL_WGRAD and eb < TOL_WGRAD


@pytest.mark.parametrize("N,H,W,Cin,Cout,K,J,slope", [(3, 16, 4, 3, 64, 3, 4, 0.2), (2, 4, 32, 6, 64, 9, 4, 0.2)])
def test_rect_dgrad_xfold(N, H, W, Cin, Cout, K, J, slope):
    """gim_conv2d_xfold_weights + gim_conv2d_dgrad_xfold called directly: J divides W only (16 x 4: one folded pixel per row)."""
    from optimalstrategiesagainstgenerativeattacks_amd import _lib
    lib = _lib.load()
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(N, H, W, Cin, device=dev(), generator=g)
    dy = torch.randn(N, H, W, Cout, device=dev(), generator=g)
    w = torch.randn(Cout, K, K, Cin, device=dev(), generator=g) / np.sqrt(K * K * Cin)     # channels-last weight memory
    sigma = torch.tensor([1.7], device=dev())
    wx = torch.empty(J * Cin * K * (K + J - 1) * Cout, device=dev())
    _lib.check(lib.gim_conv2d_xfold_weights(w.data_ptr(), wx.data_ptr(), Cout, Cin, K, J, _stream()), "xfold_weights")
    sh = _lib.GimConvShape(N, H, W, Cin, Cout, K, 0, slope)
    dx = torch.full((N, H, W, Cin), float("nan"), device=dev())
    _lib.check(lib.gim_conv2d_dgrad_xfold(dy.data_ptr(), wx.data_ptr(), sigma.data_ptr(), x.data_ptr(), dx.data_ptr(), sh, J, _stream()), "dgrad_xfold")
    xr = x.double().permute(0, 3, 1, 2).cpu().requires_grad_()
    yr = F.conv2d(F.leaky_relu(xr, slope), w.double().permute(0, 3, 1, 2).cpu() / 1.7, padding=(K - 1) // 2)
    (yr * dy.double().permute(0, 3, 1, 2).cpu()).sum().backward()
    e = relerr(nchw(dx), xr.grad)
    print("rect dgrad_xfold %s: dx %.2e" % ((N, H, W, Cin, Cout, K, J), e))
    assert e < TOL


@pytest.mark.parametrize("N,H,W,Cin,Cout,K,stride", [(2, 8, 16, 32, 64, 3, 2), (2, 16, 8, 32, 64, 3, 2), (2, 16, 4, 64, 128, 1, 2), (2, 4, 16, 32, 64, 3, 1)])
def test_rect_conv2d_infer(N, H, W, Cin, Cout, K, stride):
    """gim_conv2d_infer (bias + per-channel PReLU epilogue): the strided gather on rectangles, and stride 1 on the patch-resident loop."""
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    tag = "rectinfer%s" % ((N, H, W, Cin, Cout, K, stride),)
    x = T(pf.normal(tag + "x", (N, Cin, H, W))).float().double()       # the values the kernel sees
    w = T(pf.normal(tag + "w", (Cout, Cin, K, K)) / np.sqrt(Cin * K * K)).float().double()
    b = T(pf.normal(tag + "b", (Cout,))).float().double()
    a = T(pf.uniform(tag + "a", (Cout,))).float().double()
    ref = F.conv2d(x, w, b, stride, (K - 1) // 2)
    ref = torch.where(ref >= 0, ref, ref * a.view(1, -1, 1, 1))
    if stride == 1:
        plan = epi_plan(ops.ConvGeom.make(N, H, W, Cin, Cout, K).shape(None), 0)
        assert plan[7] & 0xff == 1, plan
    with torch.no_grad():
        got = ops.conv2d_infer(nhwc(x), w.permute(0, 2, 3, 1).contiguous().float().to(dev()), b.float().to(dev()), a.float().to(dev()), stride)
    assert tuple(got.shape) == (N, H // stride, W // stride, Cout)
    e = relerr(nchw(got), ref)
    print("rect infer %s: y %.2e" % ((N, H, W, Cin, Cout, K, stride), e))
    assert e < TOL


F16_RECT = [
    # name, (N, H, W, Cin, Cout, K, ups, pool, slope, res)
    ("f16_tap_4x8", (2, 4, 8, 32, 64, 3, 0, 0, 0.2, 1)),
    ("f16_patch_4x16", (2, 4, 16, 32, 64, 3, 0, 0, 0.2, 0)),
    ("f16_patch_16x4", (2, 16, 4, 32, 64, 3, 0, 0, 0.2, 2)),
    ("f16_patch_32x2", (2, 32, 2, 32, 64, 3, 0, 0, 0.2, 1)),
    ("f16_pool_8x16", (2, 8, 16, 32, 64, 3, 0, 1, 0.2, 0)),
    ("f16_subpix_16x8", (3, 16, 8, 32, 64, 3, 1, 0, 0.2, 0)),
]


@pytest.mark.parametrize("name,geom", F16_RECT, ids=[c[0] for c in F16_RECT])
def test_rect_fp16_path(name, geom, fp16_path):
    """The fp16 twins on rectangles: forward, dgrad on transposed weights and weight gradient all plan loop form 2.  Plain convolutions
    against fp64 on fp16-rounded operands (TOL); the folded forms, whose folded weights are rounded after folding, against the
    un-rounded reference (TOL_ROUND; the bias gradient is summed in fp32 before any rounding: TOL)."""
    ops = fp16_path
    N, H, W, Cin, Cout, K, ups, pool, slope, res = geom
    plan = rect_plan(ops, RectCase(name, geom, None, None))
    assert plan["route"] == ("plain", "t", 0) and plan["fwd"][0] == plan["dgrad_t"][0] == plan["wgrad"][0] == 2, plan
    print("rect %s %s plan %s" % (name, geom, plan))
    folded = bool(ups or pool)
    tol = {"y": TOL_ROUND, "dx": TOL_ROUND, "dw": TOL_ROUND, "db": TOL, "dres": TOL} if folded else TOL
    errs = conv_fwd_bwd(ops, "rect_" + name, N, (H, W), Cin, Cout, K, ups, bool(pool), slope, res, 1.7, tol, rnd=None if folded else r16)
    if folded:
        assert errs["y"] > 1e-6, "the fp16 path did not run"


@pytest.mark.parametrize("H,W", [(4, 16), (16, 4)])
def test_rect_pointwise_operators(H, W):
    """The pointwise kernels that take H and W, on 5 channels: ops.avg_pool2 both ways, ops.conv2d_forkpool on activated storage
    (gim_avgpool2_fwd_act going forward, gim_add_avgpool2_bwd behind the x-folded dgrad going back), the backward of a half-resolution
    residual (gim_upsample2x_bwd), gim_pad_image and gim_depth_to_space2 called directly."""
    from optimalstrategiesagainstgenerativeattacks_amd import _lib, ops
    lib = _lib.load()
    N, C, slope = 3, 5, 0.2
    tag = "rectpw%dx%d" % (H, W)
    x = T(pf.normal(tag + "x", (N, C, H, W))).requires_grad_()
    y = F.avg_pool2d(x, 2)
    r = T(pf.uniform(tag + "r", tuple(y.shape)))
    (y * r).sum().backward()
    xg = nhwc(x).requires_grad_()
    yg = ops.avg_pool2(xg)
    (yg * nhwc(r)).sum().backward()
    assert relerr(nchw(yg), y) < TOL and relerr(nchw(xg.grad), x.grad) < TOL, "avg_pool2"

    Cout = 16
    x.grad = None
    w = T(pf.normal(tag + "w", (Cout, C, 3, 3)) / np.sqrt(C * 9)).requires_grad_()
    b = T(pf.normal(tag + "b", (Cout,))).requires_grad_()
    yc, pooled = F.conv2d(F.leaky_relu(x, slope), w / 1.4, b, padding=1), F.avg_pool2d(x, 2)
    r1, r2 = T(pf.uniform(tag + "r1", tuple(yc.shape))), T(pf.uniform(tag + "r2", tuple(pooled.shape)))
    ((yc * r1).sum() + (pooled * r2).sum()).backward()
    xin = nhwc(F.leaky_relu(x, slope)).requires_grad_()          # stored activated: the pool inverts the LeakyReLU
    wg = w.detach().float().to(dev()).contiguous(memory_format=torch.channels_last).requires_grad_()
    bg = b.detach().float().to(dev()).requires_grad_()
    geom = ops.ConvGeom.make(N, H, W, C, Cout, 3, 0, slope, has_bias=True, x_act=True)
    assert ops._dgrad_route(geom, 0, True, True) == ("xfold", 4, True)
    sg, u0, v0 = torch.tensor([1.4], device=dev()), torch.zeros(Cout, device=dev()), torch.zeros(C * 9, device=dev())
    yg, act, pg = ops.conv2d_forkpool(xin, wg, bg, sg, u0, v0, slope, None, 1.0, True, slope)
    assert relerr(nchw(yg), yc) < TOL and relerr(nchw(pg), pooled) < TOL and not act, "forkpool forward"
    ((yg * nhwc(r1)).sum() + (pg * nhwc(r2)).sum()).backward()
    assert relerr(nchw(xin.grad), x.grad) < TOL, "forkpool dx"
    assert relerr(wg.grad.double().cpu(), w.grad) < TOL and relerr(bg.grad.double().cpu(), b.grad) < TOL, "forkpool dw, db"

    conv_fwd_bwd(ops, tag + "resups", N, (H, W), 16, C, 3, 0, False, slope, 2, None, TOL)     # dres: gim_upsample2x_bwd on 5 channels

    pad = 4
    xp = torch.full((N, H + 2 * pad, W + 2 * pad, C), float("nan"), device=dev())
    xs = nhwc(x)
    _lib.check(lib.gim_pad_image(xs.data_ptr(), xp.data_ptr(), N, H, W, C, pad, slope, _stream()), "pad_image")
    want = F.pad(F.leaky_relu(xs.double(), slope), (0, 0, pad, pad, pad, pad))
    assert relerr(xp, want) < ULP2, "pad_image"

    y4 = T(pf.normal(tag + "y4", (N, H, W, 4 * C))).float().to(dev())
    bias = T(pf.normal(tag + "b4", (C,))).float().to(dev())
    out = torch.full((N, 2 * H, 2 * W, C), float("nan"), device=dev())
    _lib.check(lib.gim_depth_to_space2(y4.data_ptr(), bias.data_ptr(), out.data_ptr(), N, H, W, C, slope, _stream()), "depth_to_space2")
    want = y4.double().view(N, H, W, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N, 2 * H, 2 * W, C) + bias.double()
    assert relerr(out, F.leaky_relu(want.double(), slope)) < ULP2, "depth_to_space2"
