"""Shared test helpers: portable-fill state dicts / episodes as torch tensors."""
import collections
import contextlib
import json
import os

import numpy as np
import torch

from oracle import portable_fill as pf
from tests import finish_ref as fr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def T(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def load_keys(cfg):
    with open(os.path.join(GOLDEN, "state_dict_keys.json")) as f:
        return json.load(f)[cfg]


def filled_sd(keys_and_shapes, tag, dtype=torch.float64):
    """Ordered {key: tensor} conditioned fill (see oracle/portable_fill.py)."""
    return {k: T(pf.fill_value(k, tuple(s), tag), dtype) for k, s in keys_and_shapes}


def episode(tag, B, m, n, k, c, s, d, dtype=torch.float64):
    def img(name, t):
        return T(np.clip(pf.normal("%s/%s" % (tag, name), (B, t, c, s, s)) * 0.5, -1, 1), dtype)
    return img("leaked", m), img("real", n), img("si", k), T(pf.normal(tag + "/z", (B, n, d)), dtype)


def relerr(a, b, atol=1e-12):
    """||a-b|| / (||b|| + atol*sqrt(numel)): relative L2 error with an absolute floor so that
    quantities that are mathematically zero (e.g. a conv bias grad in front of AdaIN) compare equal."""
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / (b.norm() + atol * max(b.numel(), 1) ** 0.5))


def load_npz(name):
    return np.load(os.path.join(GOLDEN, name))


def load_json(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def relerr_floor(a, b, floor):
    """||a-b|| / (||b|| + floor): for families of gradients where some members are mathematically zero
    (conv bias in front of a norm layer, attention f-bias): `floor` is set from the family's largest norm."""
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / (b.norm() + floor))


# ---- kernel family x epilogue mode cells of the forward-style convolution kernels (test_gpu_ops.py, test_gpu_fp16.py) ----
_EPI_REF = {}


def epi_plan(sh, kind):
    import ctypes
    from optimalstrategiesagainstgenerativeattacks_amd import _lib
    out = (ctypes.c_int32 * 8)()
    _lib.check(_lib.load().gim_conv_launch_plan(ctypes.byref(sh), kind, ctypes.cast(out, ctypes.c_void_p)), "plan")
    return list(out)


def epi_reference(name, N, S, Cin, Cout, r16=lambda t: t.detach()):
    """fp64 inputs and expected results of one family, computed once and shared by its modes (r16: the operand rounding of the fp16 path)."""
    import torch.nn.functional as F
    from oracle import gim_oracle as go
    if name not in _EPI_REF:
        tag = "epi" + name
        x = T(pf.normal(tag + "x", (N, Cin, S, S)))
        w = T(pf.normal(tag + "w", (Cout, Cin, 3, 3)) / np.sqrt(Cin * 9))
        b = T(pf.normal(tag + "b", (Cout,)))
        res = T(pf.normal(tag + "r", (N, Cout, S, S)))
        res_half = T(pf.normal(tag + "rh", (N, Cout, S // 2, S // 2)))
        dy = T(pf.uniform(tag + "dy", (N, Cout, S, S)))
        dpool = T(pf.uniform(tag + "dp", (N, Cin, S // 2, S // 2)))
        slope_c = T(pf.uniform(tag + "s", (Cout,)))
        sig, slope = 1.7, 0.2
        xa, wr = r16(F.leaky_relu(x, slope)).requires_grad_(), r16(w)
        y0 = F.conv2d(xa, wr, None, padding=1) / sig + b.view(1, -1, 1, 1)
        dxa, = torch.autograd.grad(y0, xa, r16(dy))
        dx = dxa * torch.where(x > 0, torch.ones_like(x), torch.full_like(x, slope))
        yi = F.conv2d(r16(x), wr, b, padding=1)
        _EPI_REF[name] = dict(x=x, w=w, b=b, res=res, res_half=res_half, dy=dy, dpool=dpool, slope_c=slope_c, sig=sig, slope=slope,
                              y0=y0.detach(), y1=(y0 + res).detach(), y2=(y0 + go.upsample2(res_half)).detach(), dx=dx,
                              dx_pool=dx + 0.25 * go.upsample2(dpool),          # + the backward of avgpool2(x) read by a second consumer
                              y5=torch.where(yi >= 0, yi, yi * slope_c.view(1, -1, 1, 1)))
    return _EPI_REF[name]


def epi_case(ops, family, mode, name, N, S, Cin, Cout, form, pm, ref, tol):
    """One (family, mode) cell: asserts the plan (loop form out[7] & 0xff, position-major rows by the skipped share in out[7] >> 8,
    the split in out[3]), then runs the mode and compares with the shared reference."""
    g = ops.ConvGeom.make(N, S, S, Cin, Cout, 3, 0, ref["slope"], has_bias=True)
    f16, split, bwd, infer = form == 2, mode == "split_k", mode[0] in "34", mode[0] == "5"
    # At these sizes the heuristic splits K to fill the chip, so every cell states its split: none (the storing epilogue), or two slices
    # for "split_k" (the atomic one).  Tile code + 20000 keeps a caller's choice on the patch-resident loop; the fp16 path takes the
    # split and no caller tile.  (The inference entry takes no overrides and never splits.)
    if not infer:
        ops._TUNE_OVERRIDE[("dgrad" if bwd else "fwd", g.key)] = ((20064 if form == 1 else 0), 2 if split else 1)
        ops._SPLITS_K.clear()
    try:
        # (mode 5: the plan query has no kind for gim_conv2d_infer; the forward plan of the same geometry names the family - plan_igemm reads
        # neither slope nor epilogue - and the entry point clamps the split to 1, so out[3] is not compared for it)
        plan = epi_plan(g.shape("dgrad" if bwd else "fwd"), (2 if f16 else 1) if bwd else 0)
        assert plan[7] & 0xff == form and (plan[7] >> 8 > 0) == pm and (infer or plan[3] == (2 if split else 1)), (family, mode, plan)
        if mode[0] == "4":
            assert ops._dgrad_route(g, 0, True, True) == ("res", 0, False)
        assert torch.cuda.is_available(), "GPU tests need an MI355X"
        dev = torch.device("cuda:0")
        nhwc = lambda t: t.detach().permute(0, 2, 3, 1).contiguous().float().to(dev)     # NCHW cpu f64 -> NHWC cuda f32
        nchw = lambda t: t.detach().permute(0, 3, 1, 2).double().cpu()
        sg = torch.tensor([ref["sig"]], device=dev)
        u0, v0 = torch.zeros(Cout, device=dev), torch.zeros(Cin * 9, device=dev)
        xg, wg = nhwc(ref["x"]).requires_grad_(bwd), ref["w"].detach().float().to(dev).contiguous(memory_format=torch.channels_last).requires_grad_()
        bg = ref["b"].float().to(dev).requires_grad_(bwd)
        if mode[0] in "012s":
            rg = {"1": nhwc(ref["res"]), "2": nhwc(ref["res_half"])}.get(mode[0])
            with torch.no_grad():
                yg = ops.conv2d(xg, wg, bg, rg, sg, None, None, 0, ref["slope"], False, mode[0] == "2")
            assert relerr(nchw(yg), ref["y" + (mode[0] if mode[0] in "12" else "0")]) < tol, (family, mode)
        elif mode[0] == "3":
            yg = ops.conv2d(xg, wg, bg, None, sg, u0, v0, 0, ref["slope"])
            (yg * nhwc(ref["dy"])).sum().backward()
            assert relerr(nchw(xg.grad), ref["dx"]) < tol, (family, mode)
        elif mode[0] == "4":
            yg, act, pg = ops.conv2d_forkpool(xg, wg, bg, sg, u0, v0, ref["slope"], None, 1.0, False, 1.0)
            ((yg * nhwc(ref["dy"])).sum() + (pg * nhwc(ref["dpool"])).sum()).backward()
            assert relerr(nchw(xg.grad), ref["dx_pool"]) < tol, (family, mode)
        else:
            with torch.no_grad():
                yg = ops.conv2d_infer(xg, wg.detach().permute(0, 2, 3, 1).contiguous(), bg, ref["slope_c"].float().to(dev))
            assert relerr(nchw(yg), ref["y5"]) < tol, (family, mode)
    finally:
        ops._TUNE_OVERRIDE.clear()
        ops._SPLITS_K.clear()


# ---- one convolution through ops.conv2d against fp64 F.conv2d autograd (test_gpu_ops.py, test_gpu_fp16.py, test_gpu_rect_maps.py) ----
class _RoundOperand(torch.autograd.Function):
    """rnd(t) going forward, the identity going back: an operand the kernel rounds when it stages it."""

    @staticmethod
    def forward(ctx, t, rnd):
        return rnd(t)

    @staticmethod
    def backward(ctx, g):
        return g, None


class _RoundCotangent(torch.autograd.Function):
    """The identity going forward, rnd(g) going back: the gradient kernels round the incoming gradient the same way."""

    @staticmethod
    def forward(ctx, t, rnd):
        ctx.rnd = rnd
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        return ctx.rnd(g), None


@contextlib.contextmanager
def tune_override(ops, g, tune):
    """ops._TUNE_OVERRIDE rows {launch kind: (tile code, split)} for the calls of geometry g, taken back on the way out."""
    for kind, ov in (tune or {}).items():
        ops._TUNE_OVERRIDE[(kind, g.key)] = ov
    ops._SPLITS_K.clear()
    try:
        yield
    finally:
        ops._TUNE_OVERRIDE.clear()
        ops._SPLITS_K.clear()


_CONV_REF = {}


def _conv_reference(tag, N, HW, Cin, Cout, K, ups, pool, slope, res, sig, rnd):
    """(x, w, b, res, y, dy) of conv_fwd_bwd in fp64, NCHW, the leaves holding their gradients of sum(y * dy)."""
    import torch.nn.functional as F
    from oracle import gim_oracle as go
    H, W = (HW, HW) if isinstance(HW, int) else HW
    x = T(pf.normal(tag + "x", (N, Cin, H >> ups, W >> ups))).requires_grad_()
    w = T(pf.normal(tag + "w", (Cout, Cin, K, K)) / np.sqrt(Cin * K * K)).requires_grad_()
    b = T(pf.normal(tag + "b", (Cout,))).requires_grad_()
    xa = F.leaky_relu(x, slope) if slope != 1.0 else x
    wr = w
    if rnd is not None:
        xa, wr = _RoundOperand.apply(xa, rnd), _RoundOperand.apply(w, rnd)
    if ups:
        xa = go.upsample2(xa)
    y = F.conv2d(xa, wr / (sig or 1.0), None, padding=(K - 1) // 2)
    if pool:
        y = F.avg_pool2d(y, 2)
    if rnd is not None:
        y = _RoundCotangent.apply(y, rnd)
    y = y + b.view(1, -1, 1, 1)
    r_ = None
    if res:
        r_ = T(pf.normal(tag + "r", (N, Cout, y.shape[2] >> (res == 2), y.shape[3] >> (res == 2)))).requires_grad_()
        y = y + (go.upsample2(r_) if res == 2 else r_)
    dy = T(pf.uniform(tag + "dy", tuple(y.shape)))
    (y * dy).sum().backward()
    return x, w, b, r_, y.detach(), dy


def conv_fwd_bwd(ops, tag, N, HW, Cin, Cout, K, ups=0, pool=False, slope=1.0, res=0, sig=None, tol=3e-5, pre=None, tune=None, rnd=None, keep_ref=False):
    """y = [avgpool2](conv(up2^ups(lrelu(x)), w / sig)) + bias [+ res] through ops.conv2d - y, dx, dw, db, dres against fp64 autograd of
    F.conv2d.  HW: the map of the unfused convolution, one int (square) or (H, W).  res: 0 none, 1 at the output's resolution, 2 at half
    of it (res_ups).  sig: None, or sigma with u = v = 0 (the plain 1 / sigma scaling of the weight gradient; the spectral term is
    test_sn_conv_sequence's).  pre: weight and bias own .grad buffers holding this value (the optimizer's bucket), so that the weight
    gradient goes through the queue and is ADDED there.  tune: launch overrides (tune_override).  rnd: the operand rounding of the fp16
    path - the reference then convolves rnd(lrelu(x)) with rnd(w) and takes the conv's gradients from rnd(dy).  tol: one bound, or one
    per compared tensor.  keep_ref: the reference of `tag` is kept for the next call (the same case run another way).  Every error is
    printed before the first is asserted; returns them."""
    ref = _CONV_REF.get(tag)
    if ref is None:
        ref = _conv_reference(tag, N, HW, Cin, Cout, K, ups, pool, slope, res, sig, rnd)
        if keep_ref:
            _CONV_REF[tag] = ref
    x, w, b, r_, y, dy = ref

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    dev = torch.device("cuda:0")
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1).contiguous().float().to(dev)     # NCHW cpu f64 -> NHWC cuda f32
    nchw = lambda t: t.detach().permute(0, 3, 1, 2).double().cpu()
    xg = nhwc(x).requires_grad_()
    wg = w.detach().float().to(dev).contiguous(memory_format=torch.channels_last).requires_grad_()
    bg = b.detach().float().to(dev).requires_grad_()
    rg = nhwc(r_).requires_grad_() if res else None
    sg = torch.tensor([sig], device=dev) if sig else None
    errs = {}
    with tune_override(ops, ops.ConvGeom.of(xg, wg, ups, slope, pool, res == 2, bg, rg, False), tune):
        yg = ops.conv2d(xg, wg, bg, rg, sg, None, None, ups, slope, pool, res == 2)
        errs["y"] = relerr(nchw(yg), y)
        # sigma given without u/v: the spectral term of the weight gradient is skipped only when sigma is None, so
        # feed u = 0 to test the plain 1/sigma scaling of wgrad here
        if sig:
            yg = ops.conv2d(xg, wg, bg, rg, sg, torch.zeros(Cout, device=dev), torch.zeros(Cin * K * K, device=dev), ups, slope, pool, res == 2)
        if pre is not None:
            wg.grad = torch.full_like(wg, pre)       # channels-last like the parameter: the bucket's memory order
            bg.grad = torch.full_like(bg, pre)
        (yg * nhwc(dy)).sum().backward()
    assert not ops.wgrad_queue.jobs, "the queue was flushed at the end of backward"
    errs["dx"] = relerr(nchw(xg.grad), x.grad)
    errs["dw"] = relerr((wg.grad - (pre or 0.0)).double().cpu(), w.grad)
    errs["db"] = relerr((bg.grad - (pre or 0.0)).double().cpu(), b.grad)
    if res:
        errs["dres"] = relerr(nchw(rg.grad), r_.grad)
    print("conv_fwd_bwd %s: %s" % (tag, " ".join("%s %.2e" % kv for kv in errs.items())))
    for k_, e in errs.items():
        assert e < (tol[k_] if isinstance(tol, dict) else tol), (k_, e)
    return errs


# ---- convolutions on maps with H != W (test_host.py asserts the plans on the CPU, test_gpu_rect_maps.py the numbers) ----
# geom = (N, H, W, Cin, Cout, K, ups, pool, slope, res) as conv_fwd_bwd reads them; tune: tune_override rows or None.
# plan: what the row is there to reach, per launch the library plans - "fwd" gim_conv2d_fwd, "dgrad" gim_conv2d_dgrad or "dgrad_t"
# gim_conv2d_dgrad_t (whichever ops._dgrad_route takes), "wgrad" gim_conv2d_wgrad_acc - as (loop form, tile rows, tile columns, skipped
# share of the K steps in 1/1000: > 0 = position-major rows), and "route" = (ops._fwd_route, ops._dgrad_route, its J).  A launch that has
# no plan kind (the "rows" and "subpixel" forwards with their weight gradients, the x-folded dgrad) has no entry.
RectCase = collections.namedtuple("RectCase", "name geom tune plan")


def rect_geom(ops, case):
    N, H, W, Cin, Cout, K, ups, pool, slope, res = case.geom
    return ops.ConvGeom.make(N, H, W, Cin, Cout, K, ups, slope, bool(pool), res == 2, True, res != 0)


def rect_plan(ops, case):
    """The plan of one row as the library and the route functions give it now, in the form of RectCase.plan."""
    g = rect_geom(ops, case)

    def row(kind, code):
        p = epi_plan(g.shape(kind), code)
        return (p[7] & 0xff, p[1], p[2], p[7] >> 8)
    with tune_override(ops, g, case.tune):
        sh = g.shape("fwd")
        fwd = ops._fwd_route(g, sh.tune_tile)
        dgrad, J, _ = ops._dgrad_route(g, sh.prec, True)
        out = {"route": (fwd, dgrad, J)}
        if fwd == "plain":
            out["fwd"] = row("fwd", 0)
        if dgrad != "xfold":
            out["dgrad_t" if dgrad == "t" else "dgrad"] = row("dgrad", 2 if dgrad == "t" else 1)
        if fwd == "plain":
            out["wgrad"] = row("wgrad", 3)
    return out


def _rc(name, geom, plan, tune=None):
    return RectCase(name, geom, tune, plan)


RECT_CASES = [
    # tap-major loop, image-major rows: a map below the 64 pixels of the patch-resident kernel
    _rc("tap_4x8", (2, 4, 8, 32, 64, 3, 0, 0, 0.2, 1),
        dict(route=("plain", "plain", 0), fwd=(0, 64, 64, 0), dgrad=(0, 128, 32, 0), wgrad=(0, 64, 128, 0))),
    _rc("tap_8x4", (2, 8, 4, 32, 64, 3, 0, 0, 0.2, 2),
        dict(route=("plain", "plain", 0), fwd=(0, 64, 64, 0), dgrad=(0, 128, 32, 0), wgrad=(0, 64, 128, 0))),
    # position-major rows (>= 32 images, <= 16 pixels): pm_perm_of orders the pixels of 2 x 8 and 8 x 2 differently
    _rc("pm_2x8", (32, 2, 8, 32, 64, 3, 0, 0, 0.2, 1),
        dict(route=("plain", "plain", 0), fwd=(0, 128, 64, 333), dgrad=(0, 128, 32, 333), wgrad=(0, 64, 128, 0))),
    _rc("pm_8x2", (32, 8, 2, 32, 64, 3, 0, 0, 0.2, 0),
        dict(route=("plain", "plain", 0), fwd=(0, 128, 64, 194), dgrad=(0, 128, 32, 194), wgrad=(0, 64, 128, 0))),
    _rc("pm_1x16", (40, 1, 16, 32, 48, 3, 0, 0, 0.2, 0),  # one tap row valid, ragged output channels
        dict(route=("plain", "plain", 0), fwd=(0, 128, 64, 667), dgrad=(0, 128, 32, 667), wgrad=(0, 64, 128, 0))),
    _rc("pm_16x1", (40, 16, 1, 32, 48, 3, 0, 0, 1.0, 1),  # one tap column valid
        dict(route=("plain", "plain", 0), fwd=(0, 128, 64, 667), dgrad=(0, 128, 32, 667), wgrad=(0, 64, 128, 0))),
    _rc("pm_1x4", (33, 1, 4, 16, 32, 3, 0, 0, 0.2, 0),  # 128 x 32 tile
        dict(route=("plain", "plain", 0), fwd=(0, 128, 32, 667), dgrad=(0, 128, 16, 667), wgrad=(0, 32, 128, 0))),
    # patch-resident loop: Wt = min(W, BM) pixels of BM / Wt + 2 patch rows
    _rc("patch_4x16", (2, 4, 16, 32, 64, 3, 0, 0, 0.2, 1),
        dict(route=("plain", "plain", 0), fwd=(1, 64, 64, 0), dgrad=(1, 64, 64, 0), wgrad=(0, 64, 128, 0))),
    _rc("patch_16x4", (2, 16, 4, 32, 64, 3, 0, 0, 0.2, 2),
        dict(route=("plain", "plain", 0), fwd=(1, 64, 64, 0), dgrad=(1, 64, 64, 0), wgrad=(0, 64, 128, 0))),
    _rc("patch_32x2", (2, 32, 2, 32, 64, 3, 0, 0, 0.2, 0),  # the narrowest legal width
        dict(route=("plain", "plain", 0), fwd=(1, 64, 64, 0), dgrad=(1, 64, 64, 0), wgrad=(0, 64, 128, 0))),
    _rc("patch_2x32", (2, 2, 32, 32, 64, 3, 0, 0, 1.0, 1),
        dict(route=("plain", "plain", 0), fwd=(1, 64, 64, 0), dgrad=(1, 64, 64, 0), wgrad=(0, 64, 128, 0))),
    _rc("patch_2x128", (1, 2, 128, 32, 64, 3, 0, 0, 0.2, 0),  # a tile is half an image row
        dict(route=("plain", "plain", 0), fwd=(1, 64, 64, 0), dgrad=(1, 64, 64, 0), wgrad=(0, 64, 128, 0))),
    _rc("patch_128x2", (1, 128, 2, 32, 64, 3, 0, 0, 0.2, 1),  # whole-row tiles at W = 2: 128 x 64
        dict(route=("plain", "plain", 0), fwd=(1, 128, 64, 0), dgrad=(1, 128, 64, 0), wgrad=(0, 64, 128, 0))),
    _rc("patch_1x64", (2, 1, 64, 32, 64, 3, 0, 0, 0.2, 0),  # H = 1: two of three patch rows out of range
        dict(route=("plain", "plain", 0), fwd=(1, 64, 64, 0), dgrad=(1, 64, 64, 0), wgrad=(0, 64, 128, 0))),
    _rc("tap_64x1", (2, 64, 1, 32, 64, 3, 0, 0, 0.2, 0),  # W = 1: the patch kernel is not allowed there
        dict(route=("plain", "plain", 0), fwd=(0, 128, 64, 0), dgrad=(0, 128, 32, 0), wgrad=(0, 64, 128, 0))),
    # 128-row patch tiles on request (tile code + 20000), one K slice
    _rc("forced_20128_64x2", (3, 64, 2, 32, 160, 3, 0, 0, 0.2, 0),
        dict(route=("plain", "plain", 0), fwd=(1, 128, 128, 0), dgrad=(1, 128, 64, 0), wgrad=(0, 128, 128, 0)), tune={"fwd": (20128, 1)}),
    _rc("forced_20641_64x2", (3, 64, 2, 32, 160, 3, 0, 0, 0.2, 1),
        dict(route=("plain", "plain", 0), fwd=(1, 64, 128, 0), dgrad=(1, 128, 64, 0), wgrad=(0, 128, 128, 0)), tune={"fwd": (20641, 1)}),
    _rc("forced_20128_4x64", (3, 4, 64, 32, 160, 3, 0, 0, 0.2, 0),
        dict(route=("plain", "plain", 0), fwd=(1, 128, 128, 0), dgrad=(1, 128, 64, 0), wgrad=(0, 128, 128, 0)), tune={"fwd": (20128, 1)}),
    _rc("forced_21264_64x2", (3, 64, 2, 32, 64, 3, 0, 0, 0.2, 0),
        dict(route=("plain", "plain", 0), fwd=(1, 128, 64, 0), dgrad=(1, 128, 64, 0), wgrad=(0, 64, 128, 0)), tune={"fwd": (21264, 1)}),
    # generic K: Cin not a multiple of 16
    _rc("genk_4x16", (2, 4, 16, 24, 64, 3, 0, 0, 0.2, 0),
        dict(route=("plain", "plain", 0), fwd=(0, 128, 64, 0), dgrad=(0, 128, 32, 0), wgrad=(0, 64, 128, 0))),
    _rc("genk_16x4", (2, 16, 4, 24, 40, 3, 0, 0, 0.2, 1),
        dict(route=("plain", "plain", 0), fwd=(0, 128, 64, 0), dgrad=(0, 128, 32, 0), wgrad=(0, 64, 128, 0))),
    # pool fold: stride-2 gather on the logical grid H/2 x W/2
    _rc("pool_8x16", (2, 8, 16, 32, 64, 3, 0, 1, 0.2, 1),
        dict(route=("plain", "plain", 0), fwd=(0, 64, 64, 0), dgrad=(0, 128, 32, 0), wgrad=(0, 64, 128, 0))),
    _rc("pool_16x8", (2, 16, 8, 32, 64, 3, 0, 1, 0.2, 0),
        dict(route=("plain", "plain", 0), fwd=(0, 64, 64, 0), dgrad=(0, 128, 32, 0), wgrad=(0, 64, 128, 0))),
    _rc("pool_2x16", (2, 2, 16, 64, 64, 3, 0, 1, 0.2, 1),  # output 1 x 8
        dict(route=("plain", "plain", 0), fwd=(0, 64, 64, 0), dgrad=(0, 64, 64, 0), wgrad=(0, 64, 128, 0))),
    _rc("pool_16x2_1x1", (2, 16, 2, 64, 64, 1, 0, 1, 1.0, 0),  # output 8 x 1
        dict(route=("plain", "plain", 0), fwd=(0, 64, 64, 0), dgrad=(0, 64, 64, 0), wgrad=(0, 64, 128, 0))),
    _rc("pool_pm_4x8", (40, 4, 8, 32, 32, 3, 0, 1, 0.2, 1),
        dict(route=("plain", "plain", 0), fwd=(0, 128, 32, 167), dgrad=(0, 128, 32, 125), wgrad=(0, 32, 128, 0))),
    _rc("pool_pm_8x4", (40, 8, 4, 32, 32, 3, 0, 1, 0.2, 0),
        dict(route=("plain", "plain", 0), fwd=(0, 128, 32, 104), dgrad=(0, 128, 32, 125), wgrad=(0, 32, 128, 0))),
    # sub-pixel form: four parity classes on the low-resolution grid H/2 x W/2
    _rc("subpix_8x16", (3, 8, 16, 32, 64, 3, 1, 0, 0.2, 1),
        dict(route=("plain", "plain", 0), fwd=(0, 128, 64, 0), dgrad=(0, 128, 32, 0), wgrad=(0, 32, 128, 0))),
    _rc("subpix_16x8", (3, 16, 8, 32, 64, 3, 1, 0, 0.2, 2),
        dict(route=("plain", "plain", 0), fwd=(0, 128, 64, 0), dgrad=(0, 128, 32, 0), wgrad=(0, 32, 128, 0))),
    _rc("subpix_pm_4x8", (33, 4, 8, 32, 64, 3, 1, 0, 0.2, 0),
        dict(route=("plain", "plain", 0), fwd=(0, 128, 64, 125), dgrad=(0, 128, 32, 167), wgrad=(0, 32, 128, 0))),
    _rc("subpix_pm_8x4", (33, 8, 4, 32, 64, 3, 1, 0, 0.2, 1),
        dict(route=("plain", "plain", 0), fwd=(0, 128, 64, 125), dgrad=(0, 128, 32, 104), wgrad=(0, 32, 128, 0))),
    _rc("subpix_9x9_2x16", (2, 2, 16, 16, 16, 9, 1, 0, 1.0, 1),  # low resolution 1 x 8
        dict(route=("plain", "plain", 0), fwd=(0, 128, 16, 0), dgrad=(0, 128, 16, 0), wgrad=(0, 32, 128, 0))),
    _rc("ups_1x1_8x2", (4, 8, 2, 32, 16, 1, 1, 0, 1.0, 0),  # 1x1 behind the upsample
        dict(route=("plain", "ups", 0), fwd=(0, 128, 16, 0), dgrad=(0, 128, 32, 0), wgrad=(0, 32, 128, 0))),
    # image layers: "rows" forward on the padded copy, x-folded dgrad where J divides W
    _rc("img_16x4", (3, 16, 4, 3, 64, 3, 0, 0, 0.2, 0),  # J = 4 = W
        dict(route=("rows", "xfold", 4))),
    _rc("img_4x32_9x9", (2, 4, 32, 6, 64, 9, 0, 0, 0.2, 0),
        dict(route=("rows", "xfold", 4))),
    _rc("img_8x16_c8", (2, 8, 16, 8, 32, 3, 0, 0, 0.2, 0),  # J = 2
        dict(route=("rows", "xfold", 2))),
    _rc("img_32x2", (3, 32, 2, 3, 64, 3, 0, 0, 0.2, 0),  # J does not divide W: transposed-weight dgrad
        dict(route=("rows", "t", 0), dgrad_t=(0, 128, 16, 0))),
    _rc("img_8x1", (2, 8, 1, 3, 64, 3, 0, 0, 1.0, 0),
        dict(route=("rows", "t", 0), dgrad_t=(0, 128, 16, 0))),
    _rc("img_out_16x8_9x9", (2, 16, 8, 64, 3, 9, 1, 0, 0.2, 0),  # stacked parity classes + depth-to-space
        dict(route=("subpixel", "plain", 0), dgrad=(0, 64, 64, 0))),
]
RECT_IDS = [c.name for c in RECT_CASES]

# Direct gim_conv2d_wgrad_acc calls on the row-resident weight gradient (tile code 20000; N, H, W, Cin, Cout, loop form of the plan):
# form 1 = the row-resident kernel in 128 x 96 tiles, rows of min(W, 16) pixels; form 0 = refused (W < 4: its narrowest instantiation walks
# rows of 4 pixels), the MFMA kernel runs instead.
RECT_WGRAD_ROW_CASES = [
    (5, 4, 16, 32, 128, 1),      # three slices of 112 pixels: they end inside an image
    (5, 16, 4, 32, 128, 1),
    (9, 2, 8, 32, 128, 1),       # two image rows per step
    (3, 1, 16, 32, 128, 1),
    (3, 64, 4, 32, 128, 1),
    (3, 4, 64, 64, 128, 1),
    (2, 2, 64, 32, 128, 1),
    (2, 1, 128, 32, 128, 1),
    (9, 8, 2, 32, 128, 0),       # H * W >= 16 with W = 2
    (3, 16, 1, 32, 128, 0),
]


def rect_wgrad_row_shape(case):
    from optimalstrategiesagainstgenerativeattacks_amd import _lib
    N, H, W, Cin, Cout, _ = case
    return _lib.GimConvShape(N, H, W, Cin, Cout, 3, 0, 0.2, 0, 0, 0, 20000, 0, 0)


def assert_rect_wgrad_row_plan(case):
    N, H, W, Cin, Cout, form = case
    plan = epi_plan(rect_wgrad_row_shape(case), 3)
    if form == 1:
        assert plan[7] == 1 and plan[1:3] == [128, 96] and plan[4] == 3 * (Cin // 32) and plan[5] == Cout // 128, (case, plan)
    else:
        assert plan[7] == 0 and plan[1:3] != [128, 96], (case, plan)


# ---- guarded device buffers and the fp64 comparison of the direct C ABI tests (test_gpu_finish_kernels.py, test_gpu_twin_entries.py) ----
TOL = 3e-5
GUARD = 64
SENTINEL = 1.25e30     # guard bands
JUNK = -7.5e28         # what an output holds before the call: an element the kernel leaves out cannot pass a comparison


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def f64(a):
    return np.asarray(a, dtype=np.float64)


def _dev_tensor(a):
    return torch.from_numpy(f32(a).reshape(-1)).to(dev())


class Guarded:
    """n floats between two guard bands, one allocation.  init: values (any shape) or None = JUNK."""

    def __init__(self, name, n, init=None):
        self.name, self.n = name, n
        self.raw = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=dev())
        self.t = self.raw[GUARD:GUARD + n]
        self.fill(init)

    def fill(self, init=None):
        if init is None:
            self.t.fill_(JUNK)
        else:
            self.t.copy_(_dev_tensor(init))

    @property
    def ptr(self):
        return self.t.data_ptr()

    def np(self):
        return self.t.double().cpu().numpy()

    def intact(self):
        lo, hi = self.raw[:GUARD], self.raw[GUARD + self.n:]
        return bool((lo == SENTINEL).all()) and bool((hi == SENTINEL).all())


class Pool(list):
    def new(self, name, n, init=None):
        self.append(Guarded(name, n, init))
        return self[-1]

    def check(self, what=""):
        torch.cuda.synchronize()
        broken = [g.name for g in self if not g.intact()]
        assert not broken, "%s wrote outside %s" % (what, broken)


_WORST = {}


def _report(group, what, got, ref, bound=None, scale=None, m=None, l2_ref=None):
    """Prints and returns (relative L2 error, largest |got - ref| / bound); bound = gamma(m) * scale unless given.  Where the bound
    is zero the values must be equal.  l2_ref: another reference for the L2 error (the chained one of the power iterations)."""
    got, ref = f64(got).reshape(-1), f64(ref).reshape(-1)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), what
    if bound is None:
        bound = fr.gamma(m) * f64(scale).reshape(-1)
    bound = np.broadcast_to(f64(bound).reshape(-1), ref.shape)
    err = np.abs(got - ref)
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    if (err[~pos] > 0).any():
        ratio = float("inf")
    l2 = relerr(torch.from_numpy(got), torch.from_numpy(ref if l2_ref is None else f64(l2_ref).reshape(-1)))
    w = _WORST.setdefault(group, [0.0, 0.0])
    w[0], w[1] = max(w[0], l2), max(w[1], ratio)
    print("FINISH %s %s: L2 %.3e (TOL %.0e)  elementwise error / bound %.4f%s   [group worst so far: %.3e, %.4f]"
          % (group, what, l2, TOL, ratio, "" if m is None else " (m = %d)" % m, w[0], w[1]))
    return l2, ratio


def _check(group, what, got, ref, bound=None, scale=None, m=None, l2_ref=None):
    l2, ratio = _report(group, what, got, ref, bound, scale, m, l2_ref)
    assert l2 < TOL, (what, "L2", l2)
    assert ratio <= 1.0, (what, "elementwise error / bound", ratio)
