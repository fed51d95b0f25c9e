"""CPU tests of tests/finish_ref.py, the fp64 yardstick of tests/test_gpu_finish_kernels.py: the power iteration against the
oracle's restatement of torch's spectral-norm hook, the finish against fp64 autograd through that hook, the un-folds against
autograd through the weight fold, the un-padding against slicing."""
import numpy as np
import pytest
import torch

from oracle import gim_oracle as go
from oracle import portable_fill as pf
from tests import finish_ref as fr
from tests.helpers import T

SHAPES = [(1, 1, 1), (4, 1, 3), (6, 4, 3), (65, 7, 1), (5, 3, 2), (3, 8, 9)]     # (Cout, Cin, K)


def _sd(tag, Cout, Cin, K):
    return {"weight_orig": T(pf.fill_value("weight_orig", (Cout, Cin, K, K), tag)),
            "weight_u": T(pf.fill_value("weight_u", (Cout,), tag)),
            "weight_v": T(pf.fill_value("weight_v", (Cin * K * K,), tag))}


def _mem(w):
    """[Cout][Cin][K][K] torch tensor -> [Cout][K][K][Cin] numpy (the layout the kernels read)."""
    return w.detach().permute(0, 2, 3, 1).contiguous().numpy()


def _close(a, b, tol=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and float(np.abs(a - b).max()) <= tol * max(1.0, float(np.abs(b).max()))


@pytest.mark.parametrize("shape", SHAPES)
def test_power_iteration_follows_the_oracle_hook(shape):
    Cout, Cin, K = shape
    sd = _sd("fr_pi%s" % (shape,), Cout, Cin, K)
    W = _mem(sd["weight_orig"])
    u, v = sd["weight_u"].numpy().copy(), sd["weight_v"].numpy().copy()
    for rnd, training in enumerate((True, True, False)):
        before = (sd["weight_u"].clone(), sd["weight_v"].clone())
        wn = go.sn_weight(sd, "", training)
        i = int(sd["weight_orig"].abs().argmax())
        sigma_oracle = float(sd["weight_orig"].reshape(-1)[i] / wn.reshape(-1)[i])
        sigma, u, v, S = fr.power_iteration(W, u, v, training)
        assert _close(sigma, sigma_oracle), (rnd, sigma, sigma_oracle)
        assert _close(u, sd["weight_u"].numpy()) and _close(v, sd["weight_v"].numpy()), rnd
        assert S >= abs(sigma) > 0
        if not training:
            assert torch.equal(before[0], sd["weight_u"]) and torch.equal(before[1], sd["weight_v"])
    # the stage-wise form is the same round, fed the exact intermediate results
    s0, u0, v0, _ = fr.power_iteration(W, sd["weight_u"].numpy(), sd["weight_v"].numpy(), True)
    v_ref, v_b, u_ref, u_b, s_ref, S = fr.power_iteration_stages(W, sd["weight_u"].numpy(), v0, u0)
    assert _close(v_ref, v0) and _close(u_ref, u0) and _close(s_ref, s0)
    assert (v_b > 0).all() and (u_b > 0).all() and S >= abs(s_ref)


def test_power_iteration_of_a_zero_weight_is_zero_and_a_short_vector_is_refused():
    W = np.zeros((5, 2, 2, 3))
    u, v = np.full(5, 5 ** -0.5), np.full(12, 12 ** -0.5)
    with pytest.raises(AssertionError):
        fr.power_iteration(W, u, v, True)
    sigma, u1, v1, S = fr.power_iteration(W, u, v, True, degenerate_ok=True)
    assert sigma == 0.0 and S == 0.0 and not u1.any() and not v1.any()
    # F.normalize with the same eps gives the same zeros
    assert not torch.nn.functional.normalize(torch.zeros(12, dtype=torch.float64), dim=0, eps=1e-12).any()


@pytest.mark.parametrize("shape", SHAPES)
def test_finish_is_the_gradient_through_the_hook(shape):
    Cout, Cin, K = shape
    tag = "fr_fin%s" % (shape,)
    sd = _sd(tag, Cout, Cin, K)
    go.sn_weight(sd, "", True)      # a real spectral state
    sd["weight_orig"].requires_grad_()
    R = T(pf.normal(tag + "R", (Cout, Cin, K, K)))
    (R * go.sn_weight(sd, "", False)).sum().backward()
    W = _mem(sd["weight_orig"])
    u, v = sd["weight_u"].numpy(), sd["weight_v"].numpy()
    sigma = fr.power_iteration(W, u, v, False)[0]
    dw, scale = fr.finish(_mem(R), W, sigma, u, v)
    assert _close(dw, _mem(sd["weight_orig"].grad), 1e-11)
    assert (scale >= np.abs(dw) * (1 - 1e-12)).all()
    # g_abs widens the scale, never the value
    dw2, scale2 = fr.finish(_mem(R), W, sigma, u, v, g_abs=2 * np.abs(_mem(R)))
    assert np.array_equal(dw, dw2) and (scale2 >= scale).all()


def _fold(wp):
    """F[co][a][b][ci] = sum over dh, dw in {0, 1} of W[co][a - dh][b - dw][ci] for W [Cout][K][K][Cin] (the four-shift sum of
    tests/test_gpu_ops.py::_host_fold), differentiable."""
    Cout, K, _, Cin = wp.shape
    f = torch.zeros(Cout, K + 1, K + 1, Cin, dtype=wp.dtype)
    for dh in (0, 1):
        for dw in (0, 1):
            f = f + torch.nn.functional.pad(wp, (0, 0, dw, 1 - dw, dh, 1 - dh))
    return f


@pytest.mark.parametrize("shape", SHAPES)
def test_unfold_codes_1_and_2_are_the_gradient_through_the_fold(shape):
    Cout, Cin, K = shape
    tag = "fr_unf%s" % (shape,)
    wp = T(pf.normal(tag + "w", (Cout, K, K, Cin))).requires_grad_()
    # the fold itself, against the definition element by element
    f = _fold(wp).detach().numpy()
    w = wp.detach().numpy()
    for a in range(K + 1):
        for b in range(K + 1):
            want = sum(w[:, a - dh, b - dw, :] for dh in (0, 1) for dw in (0, 1) if 0 <= a - dh < K and 0 <= b - dw < K)
            assert _close(f[:, a, b, :], want)
    dF = T(pf.normal(tag + "dF", (Cout, K + 1, K + 1, Cin)))
    # code 1: the pooled convolution reads 0.25 F
    (dF * (0.25 * _fold(wp))).sum().backward()
    g, ga = fr.unfold(dF.numpy().reshape(-1), Cout, Cin, K, 1)
    assert _close(g, wp.grad.numpy()) and (ga >= np.abs(g) * (1 - 1e-12)).all()
    # code 2: the sub-pixel convolution reads F, and its gradient arrives transposed and flipped, G[ci][K-a][K-b][co]
    wp.grad = None
    (dF * _fold(wp)).sum().backward()
    G = np.zeros((Cin, K + 1, K + 1, Cout))
    d = dF.numpy()
    for a in range(K + 1):
        for b in range(K + 1):
            G[:, K - a, K - b, :] = d[:, a, b, :].T
    g, ga = fr.unfold(G.reshape(-1), Cout, Cin, K, 2)
    assert _close(g, wp.grad.numpy()) and (ga >= np.abs(g) * (1 - 1e-12)).all()
    assert _close(ga, fr.unfold(np.abs(G).reshape(-1), Cout, Cin, K, 2)[0])


@pytest.mark.parametrize("shape", SHAPES)
def test_unfold_codes_0_and_3(shape):
    Cout, Cin, K = shape
    tag = "fr_pad%s" % (shape,)
    g0 = pf.normal(tag, (Cout, K, K, Cin))
    g, ga = fr.unfold(g0.reshape(-1), Cout, Cin, K, 0)
    assert np.array_equal(g, g0) and np.array_equal(ga, np.abs(g0))
    rp = fr.row_pad(K, Cin)
    assert rp % 16 == 0 and 0 <= rp - K * Cin < 16
    slot = pf.normal(tag + "slot", (Cout, K, rp))      # padding columns hold junk: they must not be read
    g, ga = fr.unfold(slot.reshape(-1), Cout, Cin, K, 3)
    assert np.array_equal(g, slot[:, :, :K * Cin].reshape(Cout, K, K, Cin)) and np.array_equal(ga, np.abs(g))
    assert fr.src_size(Cout, Cin, K, 3) == slot.size
    with pytest.raises(AssertionError):
        fr.unfold(slot.reshape(-1)[:-1], Cout, Cin, K, 3)


def test_gamma_is_highams():
    u = 2.0 ** -24
    assert fr.gamma(1) == u / (1 - u) and fr.gamma(3) == 3 * u / (1 - 3 * u)
    assert fr.gamma(36864 + 8) < 2.3e-3
