"""Host side of the strided training convolution (gim_conv2d_strided_fwd / _dgrad / _wgrad, ops.conv2d_strided): the entry points are
declared, bound and exported, every argument check answers without a GPU, the planned K extents are the convolution's own taps, and -
in torch fp64 on the CPU, independent of any kernel - the two identities the launches rest on: a stride-2 convolution is the even-
position subsample of the stride-1 one, and its input gradient is the four-parity-class sum of the header comment.  No GPU."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ("gim_conv2d_strided_fwd", "gim_conv2d_strided_dgrad", "gim_conv2d_strided_wgrad", "gim_conv2d_strided_wgrad_workspace",
               "gim_conv2d_strided_plan")


def _lib_loaded():
    import __graft_entry__
    from optimalstrategiesagainstgenerativeattacks_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        __graft_entry__.build()
    return _lib, _lib.load()


def test_new_entry_points_are_declared_bound_and_exported():
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    _lib, lib = _lib_loaded()
    header = open(os.path.join(ROOT, "include", "gim_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), name
    # the shape is gim_conv2d_infer's struct: the header gained no struct, gim_conv_shape is what it was
    assert header.count("typedef struct") == 6 and ctypes.sizeof(_lib.GimConvShape) == 68 and ctypes.sizeof(_lib.GimInferConv) == 28
    assert hasattr(ops, "conv2d_strided") and hasattr(ops, "ConvStridedFn")
    assert hasattr(ops, "subsample2") and "gim_subsample2_fwd" in _lib.SIGNATURES      # the old route stays


def test_entry_points_check_their_arguments_before_any_launch():
    """Every refusal comes back from the host with the entry point's name in the message; the pointers are NULL throughout, so a check
    that regressed would leave a kernel no address to touch."""
    _lib, lib = _lib_loaded()
    n = None

    def shape(N=2, H=8, W=8, Cin=16, Cout=32, KH=3, stride=2):
        return ctypes.byref(_lib.GimInferConv(N, H, W, Cin, Cout, KH, stride))
    out = (ctypes.c_int32 * 16)()
    nbytes = ctypes.c_int64(0)
    calls = {
        "conv2d_strided_fwd": lambda s: lib.gim_conv2d_strided_fwd(n, n, n, n, s, n),
        "conv2d_strided_dgrad": lambda s: lib.gim_conv2d_strided_dgrad(n, n, n, s, 0, n),
        "conv2d_strided_wgrad": lambda s: lib.gim_conv2d_strided_wgrad(n, n, n, n, s, 0, n, n),
    }
    bad = (("KH must be 1 or 3", dict(KH=5)), ("stride must be 1 or 2", dict(stride=3)), ("powers of two >= 2", dict(H=1)),
           ("powers of two >= 2", dict(W=12)), ("non-positive", dict(Cin=0)))
    for name, call in calls.items():
        assert call(shape()) < 0 and b"null pointer" in lib.gim_last_error() and name.encode() in lib.gim_last_error(), name
        assert call(None) < 0 and b"null shape" in lib.gim_last_error(), name
        for msg, kw in bad:
            assert call(shape(**kw)) < 0, (name, kw)
            err = lib.gim_last_error()
            assert name.encode() in err and msg.encode() in err, (name, kw, err)
    # the queries: a bad shape, a missing output
    assert lib.gim_conv2d_strided_wgrad_workspace(shape(KH=5), ctypes.byref(nbytes)) < 0
    assert b"conv2d_strided_wgrad_workspace" in lib.gim_last_error()
    assert lib.gim_conv2d_strided_wgrad_workspace(shape(), None) < 0
    assert lib.gim_conv2d_strided_plan(shape(stride=3), 0, ctypes.cast(out, ctypes.c_void_p)) < 0
    assert lib.gim_conv2d_strided_plan(shape(), 3, ctypes.cast(out, ctypes.c_void_p)) < 0
    assert lib.gim_conv2d_strided_plan(shape(), 0, None) < 0
    # one image beyond the 32-bit buffer-offset range cannot be halved
    assert calls["conv2d_strided_fwd"](shape(N=1, H=4096, W=4096, Cin=64, Cout=64)) < 0 and b"2 GiB" in lib.gim_last_error()


def test_ops_conv2d_strided_refuses_what_it_cannot_run():
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    x, w = torch.zeros(2, 8, 8, 4), torch.zeros(8, 3, 3, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.conv2d_strided(x, w)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.conv2d_strided(x.double(), w.double())
    # the weight forms: [Cout, KH, KH, Cin] as it stands, a channels-last [Cout, Cin, KH, KH] parameter through its storage view
    st, logical = ops._strided_weight(torch.zeros(8, 3, 3, 4), 4)
    assert not logical and tuple(st.shape) == (8, 3, 3, 4)
    p = torch.zeros(8, 4, 3, 3).contiguous(memory_format=torch.channels_last)
    st, logical = ops._strided_weight(p, 4)
    assert logical and tuple(st.shape) == (8, 3, 3, 4) and st.is_contiguous() and st.data_ptr() == p.data_ptr()
    # Cin == KH: both shapes fit, the memory order decides
    p3 = torch.arange(16 * 27, dtype=torch.float32).view(16, 3, 3, 3)
    assert ops._strided_weight(p3, 3)[1] is False
    assert ops._strided_weight(p3.permute(0, 3, 1, 2), 3)[1] is True
    for bad in (torch.zeros(8, 3, 3, 5), torch.zeros(8, 4, 3, 2), torch.zeros(8, 36)):
        with pytest.raises(RuntimeError, match="conv2d_strided"):
            ops._strided_weight(bad, 4)


def _plan(lib, _lib, kind, **kw):
    out = (ctypes.c_int32 * 16)()
    sh = _lib.GimInferConv(kw.get("N", 2), kw.get("H", 8), kw.get("W", 8), kw.get("Cin", 16), kw.get("Cout", 32), kw.get("KH", 3), 2)
    _lib.check(lib.gim_conv2d_strided_plan(ctypes.byref(sh), kind, ctypes.cast(out, ctypes.c_void_p)), "conv2d_strided_plan")
    return [list(out[4 * i:4 * i + 4]) for i in range(4)]


def test_planned_k_extent_is_the_convolutions_own_taps():
    """One shape per kind: the K the launches run over is KH^2 * C in total - 9 taps over the four dgrad classes, as 1 / 2 / 2 / 4; not
    the 16 of a zero-padded 4 x 4 fold, not the 36 of a full-resolution convolution behind a subsample."""
    _lib, lib = _lib_loaded()
    Cin, Cout = 16, 32
    fwd = _plan(lib, _lib, 0)
    assert fwd[0][0] == 9 * Cin and fwd[0][3] == 1 and fwd[1:] == [[-1] * 4] * 3         # one launch, never split
    dg = _plan(lib, _lib, 1)
    assert [r[0] for r in dg] == [1 * Cout, 2 * Cout, 2 * Cout, 4 * Cout] and sum(r[0] for r in dg) == 9 * Cout
    assert all(r[1] > 0 and r[2] > 0 and r[3] >= 1 for r in dg)
    wg = _plan(lib, _lib, 2)
    assert wg[0][0] == 9 * Cin and wg[1:] == [[-1] * 4] * 3
    # the 1x1 shortcut: one class with one tap, three without
    dg1 = _plan(lib, _lib, 1, KH=1)
    assert [r[0] for r in dg1] == [Cout, 0, 0, 0] and dg1[1] == [0, 0, 0, 0]
    assert _plan(lib, _lib, 0, KH=1)[0][0] == Cin and _plan(lib, _lib, 2, KH=1)[0][0] == Cin
    # the workspace of the deterministic combine: whole slabs of dw and of dbias
    nbytes = ctypes.c_int64(0)
    sh = _lib.GimInferConv(2, 8, 8, Cin, Cout, 3, 2)
    _lib.check(lib.gim_conv2d_strided_wgrad_workspace(ctypes.byref(sh), ctypes.byref(nbytes)), "workspace")
    assert nbytes.value > 0 and nbytes.value % (4 * (Cout * 9 * Cin + Cout)) == 0


def _dx_by_classes(dy, w, H, W):
    """dx of conv2d(x, w, stride=2, padding=(K-1)/2) from dy by the class formula, written with slices: dx[iy, ix] collects the taps
    (a, b) with (iy + pad - a), (ix + pad - b) even; oy = (iy + pad - a) / 2 must lie in [0, Ho).  dy [N, Co, Ho, Wo], w [Co, Ci, K, K]."""
    K, pad = w.shape[2], (w.shape[2] - 1) // 2
    N, Ho, Wo = dy.shape[0], H // 2, W // 2
    dx = torch.zeros(N, w.shape[1], H, W, dtype=dy.dtype)
    taps = {}
    for py in (0, 1):
        for px in (0, 1):
            n_taps = 0
            for a in range(K):
                for b in range(K):
                    if (py + pad - a) % 2 or (px + pad - b) % 2:
                        continue
                    n_taps += 1
                    sy, sx = (py + pad - a) // 2, (px + pad - b) // 2        # oy = u + sy for dx row 2 u + py
                    u0, u1 = max(0, -sy), min(Ho, Ho - sy)                    # the rows u with oy in range: the boundary row drops out
                    v0, v1 = max(0, -sx), min(Wo, Wo - sx)
                    if u0 >= u1 or v0 >= v1:
                        continue
                    contrib = torch.einsum("nouv,oc->ncuv", dy[:, :, u0 + sy:u1 + sy, v0 + sx:v1 + sx], w[:, :, a, b])
                    dx[:, :, 2 * u0 + py:2 * u1 + py:2, 2 * v0 + px:2 * v1 + px:2] += contrib
            taps[(py, px)] = n_taps
    return dx, taps


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("HW", [(2, 2), (4, 8), (8, 8)], ids=["2x2", "4x8", "8x8"])
def test_stride2_identities_in_fp64(K, HW):
    H, W = HW
    g = torch.Generator().manual_seed(100 * K + H + W)
    x = torch.randn(3, 5, H, W, dtype=torch.float64, generator=g, requires_grad=True)
    w = torch.randn(4, 5, K, K, dtype=torch.float64, generator=g)
    pad = (K - 1) // 2
    y2 = F.conv2d(x, w, stride=2, padding=pad)
    assert tuple(y2.shape) == (3, 4, H // 2, W // 2)
    assert torch.allclose(y2, F.conv2d(x, w, stride=1, padding=pad)[..., ::2, ::2], rtol=0, atol=1e-12)
    dy = torch.randn(y2.shape, dtype=torch.float64, generator=g)
    (dx_ref,) = torch.autograd.grad(y2, x, dy)
    dx, taps = _dx_by_classes(dy, w, H, W)
    assert taps == ({(0, 0): 1, (0, 1): 2, (1, 0): 2, (1, 1): 4} if K == 3 else {(0, 0): 1, (0, 1): 0, (1, 0): 0, (1, 1): 0})
    assert torch.allclose(dx, dx_ref, rtol=0, atol=1e-12)
    if K == 1:      # three classes are zeros
        assert not dx[:, :, 1::2].any() and not dx[:, :, :, 1::2].any()
