"""Shared test helpers: portable-fill state dicts / episodes as torch tensors."""
import json
import os

import numpy as np
import torch

from oracle import portable_fill as pf

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
