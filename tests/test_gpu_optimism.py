"""Optimistic Adam on the GPU: gim_adam_optimism (csrc/oadam.hip) at the C ABI against the fp64 restatement of tests/oadam_ref.py,
FusedAdam's optimistic step (recurrence, launch order in front of the average, re-home, refusals, skipped step), the bilinear
game on the device, and the trainers (first step doubled, checkpoints, resume with and without the entry, the Gaussian game).

Bounds, u = 2^-24.  hipcc keeps fp32 divide and sqrt correctly rounded (its default; the library is not built with fast-math), so
neither needs an ulp beyond the count.  All references are fp64 on the float32 values the kernel reads: m, v, p, prev, lr, omega, eps
and the float32 bc1, bc2s.

D, the direction: d^ = fl(fl(m / bc1) / fl(fl(fl(sqrt v) / bc2s) + eps)).  The denominator carries three roundings (eps > 0 only
shrinks their share), the numerator one, the quotient one: |d^ - d| <= 5 u |d| + O(u^2), taken as 6 u |d|.

C, the correction: p^' = fl(p - fl(lw * fl(d^ - prev))), lw = fl(lr * omega).  Three roundings on the product (two when the compiler
contracts to a fused multiply-add) and the one of the result, on top of D: |p^' - p'| <= u |p'| + lr omega u (6 |d| + 4 |d - prev|),
the 4 again with one for the second-order terms.  Against the RETURNED prev, which must be the d^ that went into the update, the
6 |d| term is gone: |p^' - (p - lr omega (prev^' - prev))| <= u |p'| + 4 u lr omega |prev^' - prev|.

A, Adam's own update in adam_kernel: p_a = fl(p0 - fl(fl(lr / bc1) * fl(m / denom))), denom as above: six roundings on the product,
taken as 7, and the one of the result.  A whole optimistic step of FusedAdam, p0 -> p', against p0 - lr (d + omega (d - prev)):
u (|p_a| + |p'|) + u lr (7 |d| + omega (6 |d| + 4 |d - prev|)), with |p_a| <= |p0| + 1.01 lr |d|.  With beta1 = 0 at t = 1, bc1 = 1
and lr / bc1, m / bc1 are exact: Adam's direction is d^ itself.  Derived, not measured.  (The u |p'| of the last rounding is
sharp - half an ulp of a value just above a power of two - so over millions of elements the worst error / bound comes close to 1.)"""
import os
import tempfile

import numpy as np
import pytest
import torch

from oracle import portable_fill as pf
from tests import oadam_ref as ref
from tests.helpers import Guarded, T, episode, filled_sd, load_json, load_keys

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
GRID_PASS = 4096 * 256 * 4      # floats one pass of the capped grid covers (adam.hip's launch shape)
SIZES = [1, 3, 4, 5, 255, 1024, 1025, GRID_PASS + 1029]   # the last: the grid-stride loop runs twice and leaves a tail of one
OMEGAS = [0.5, 1.0]
BETAS = [(0.0, 0.99), (0.5, 0.9)]
STEPS = [1, 1000]
EPS = 1e-8
SC_LAST_OVERFLOW = 7            # include/gim_hip.h, the scaler's words


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _lib():
    from optimalstrategiesagainstgenerativeattacks_amd import _lib as L
    return L.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    """The 32-bit patterns of a float32 device tensor, on the host."""
    return t.detach().contiguous().view(torch.int32).cpu().numpy().copy()


def _f64(a):
    return np.asarray(a, np.float32).astype(np.float64)


# ---- the bounds of the docstring -------------------------------------------------------------------------------------------------
def direction_bound(d):
    return 6 * U * np.abs(d)


def correction_bound(p_new, d, prev, lr, omega):
    return U * np.abs(p_new) + _f64(lr) * omega * U * (6 * np.abs(d) + 4 * np.abs(d - prev))


def consistency_bound(p_new, prev_new, prev, lr, omega):
    return U * np.abs(p_new) + 4 * U * _f64(lr) * omega * np.abs(prev_new - prev)


def step_bound(p0, p_new, d, prev, lr, omega):
    lr = _f64(lr)
    return U * (np.abs(p0) + 1.01 * lr * np.abs(d) + np.abs(p_new)) + U * lr * (7 * np.abs(d) + omega * (6 * np.abs(d) + 4 * np.abs(d - prev)))


def _worst(err, bound):
    err, bound = np.asarray(err).reshape(-1), np.asarray(bound).reshape(-1)
    if (err[bound == 0] > 0).any():
        return float("inf")
    pos = bound > 0
    return float((err[pos] / bound[pos]).max()) if pos.any() else 0.0


# ---- segment tables --------------------------------------------------------------------------------------------------------------
def _tables(n):
    """name -> (segment ends, learning rates): one segment; two with distinct rates; ragged: the first ends at an index = 1 mod 4 and,
    where there is room, the second at one = 3 mod 4, so that vectors straddle two segments."""
    out = {"one": ([n], [0.05])}
    out["two"] = ([max(1, n // 2), n], [0.05, 0.0125])
    if n >= 16:
        e1 = 4 * (n // 8) + 1
        e2 = 4 * (n // 6) + 3
        assert e1 % 4 == 1 and e2 % 4 == 3 and e1 < e2 < n
        out["ragged"] = ([e1, e2, n], [0.05, 0.0125, 0.2])
    else:
        out["ragged"] = ([1, n], [0.05, 0.0125])      # 1 = 1 mod 4; n = 1: the second segment is empty
    return out


def _lr_per_element(ends, lrs):
    return np.repeat(np.asarray(lrs, np.float32), np.diff([0] + list(ends)))


class _Call:
    """The device-side arguments of one gim_adam_optimism call, kept alive."""

    def __init__(self, ends, lrs, step, words=None):
        self.seg = torch.tensor(ends, dtype=torch.int64, device=dev())
        self.lr = torch.tensor(lrs, dtype=torch.float32, device=dev())
        self.step = torch.tensor([step], dtype=torch.int32, device=dev())
        self.words = None if words is None else torch.from_numpy(np.asarray(words, np.int32)).to(dev())
        self.n_seg = len(ends)

    def run(self, p, prev, m, v, n, betas, omega):
        lib = _lib()
        rc = lib.gim_adam_optimism(p.ptr, prev.ptr, m.ptr, v.ptr, n, self.seg.data_ptr(), self.lr.data_ptr(), self.n_seg, betas[0],
                                   betas[1], EPS, omega, self.step.data_ptr(), None if self.words is None else self.words.data_ptr(),
                                   _stream())
        assert rc == 0, lib.gim_last_error()
        torch.cuda.synchronize()


def _inputs(n, seed):
    """m ~ N(0, 1), v = g^2 + 1e-3 (d of order 1), p and prev ~ N(0, 1), float32."""
    rng = np.random.default_rng(seed)
    m = rng.standard_normal(n).astype(np.float32)
    v = (rng.standard_normal(n) ** 2 + 1e-3).astype(np.float32)
    p = rng.standard_normal(n).astype(np.float32)
    prev = rng.standard_normal(n).astype(np.float32)
    return m, v, p, prev


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the kernel at the C ABI
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("betas", BETAS, ids=lambda b: "b%g_%g" % b)
@pytest.mark.parametrize("n", SIZES)
def test_optimism_kernel(n, betas, step):
    m0, v0, p0, prev0 = _inputs(n, 3000 + n % 9973)
    m, v, p, prev = Guarded("m", n, m0), Guarded("v", n, v0), Guarded("p", n), Guarded("prev", n)
    m_bits, v_bits = _bits(m.t), _bits(v.t)
    d_ref = ref.direction(m0, v0, betas[0], betas[1], EPS, step)
    if n >= 255:
        assert 0.05 < float(np.abs(d_ref).mean()) < 50, "d is not of order 1"
    for name, (ends, lrs) in _tables(n).items():
        call = _Call(ends, lrs, step)
        lr = _lr_per_element(ends, lrs)
        for omega in OMEGAS:
            p.fill(p0)
            prev.fill(prev0)
            call.run(p, prev, m, v, n, betas, omega)
            got_p, got_prev = p.np(), prev.np()
            p_ref = ref.correction(p0, prev0, d_ref, lr, omega)
            r_d = _worst(np.abs(got_prev - d_ref), direction_bound(d_ref))
            r_p = _worst(np.abs(got_p - p_ref), correction_bound(p_ref, d_ref, _f64(prev0), lr, omega))
            again = ref.correction(p0, prev0, got_prev, lr, omega)      # the update recomputed from the returned prev
            r_c = _worst(np.abs(got_p - again), consistency_bound(again, got_prev, _f64(prev0), lr, omega))
            print("optimism n %d betas %s t %d table %s omega %g: error / bound  prev %.3f  p %.3f  p from returned prev %.3f"
                  % (n, betas, step, name, omega, r_d, r_p, r_c))
            assert r_d <= 1.0 and r_p <= 1.0 and r_c <= 1.0, (n, betas, step, name, omega, r_d, r_p, r_c)
            moved = np.abs(got_p - _f64(p0)) > 0
            assert moved.mean() > 0.9, "the correction did not move the parameters"
            assert all(g.intact() for g in (m, v, p, prev)), "guard bands"
            assert np.array_equal(_bits(m.t), m_bits) and np.array_equal(_bits(v.t), v_bits), "the moments are only read"


# ------------------------------------------------------------------------------------------------------------------------------
# 2. omega = 0 records only   3. the guard
# ------------------------------------------------------------------------------------------------------------------------------
def test_omega_zero_records_the_direction_only():
    n, betas, step = 1029, (0.5, 0.9), 7
    m0, v0, p0, prev0 = _inputs(n, 11)
    m, v, p, prev = Guarded("m", n, m0), Guarded("v", n, v0), Guarded("p", n, p0), Guarded("prev", n, prev0)
    ends, lrs = _tables(n)["ragged"]
    call = _Call(ends, lrs, step)
    call.run(p, prev, m, v, n, betas, 1.0)
    want_prev = _bits(prev.t)
    p.fill(p0)
    prev.fill(prev0)
    p_bits = _bits(p.raw)
    call.run(p, prev, m, v, n, betas, 0.0)
    assert np.array_equal(_bits(p.raw), p_bits), "omega = 0 touched p"
    assert np.array_equal(_bits(prev.t), want_prev), "omega = 0 records the d of an omega = 1 launch"
    assert prev.intact()
    # no applied step, no direction: every workgroup returns while the counter is 0
    prev.fill(prev0)
    before = _bits(prev.raw)
    for omega in (0.0, 1.0):
        _Call(ends, lrs, 0).run(p, prev, m, v, n, betas, omega)
        assert np.array_equal(_bits(p.raw), p_bits) and np.array_equal(_bits(prev.raw), before), "a launch at step 0 wrote"


@pytest.mark.parametrize("n", [5, 1029])
def test_guarded_launch_follows_the_scalers_last_word(n):
    betas, step = (0.0, 0.99), 3
    m0, v0, p0, prev0 = _inputs(n, 12)
    m, v, p, prev = Guarded("m", n, m0), Guarded("v", n, v0), Guarded("p", n, p0), Guarded("prev", n, prev0)
    ends, lrs = _tables(n)["two"]
    words_host = np.array([0x45800000, 0x39800000, 2000, 5, 0, 3, 0x3F800000, 1], dtype=np.int32)
    for omega in (1.0, 0.0):
        p.fill(p0)
        prev.fill(prev0)
        before = _bits(p.raw), _bits(prev.raw)
        skipped = _Call(ends, lrs, step, words_host)
        skipped.run(p, prev, m, v, n, betas, omega)
        assert np.array_equal(_bits(p.raw), before[0]) and np.array_equal(_bits(prev.raw), before[1]), "a skipped step was corrected"
        assert np.array_equal(skipped.words.cpu().numpy(), words_host), "the scaler's words are only read"
        clear = words_host.copy()
        clear[SC_LAST_OVERFLOW] = 0
        applied = _Call(ends, lrs, step, clear)
        applied.run(p, prev, m, v, n, betas, omega)
        guarded = _bits(p.t), _bits(prev.t)
        assert np.array_equal(applied.words.cpu().numpy(), clear)
        p.fill(p0)
        prev.fill(prev0)
        _Call(ends, lrs, step).run(p, prev, m, v, n, betas, omega)      # scaler_state = NULL
        assert np.array_equal(_bits(p.t), guarded[0]) and np.array_equal(_bits(prev.t), guarded[1]), \
            "the guarded correction is the plain one when the step was applied"
        assert not np.array_equal(guarded[1], _bits(torch.from_numpy(prev0))), "the applied launch did not write prev"
        assert (omega == 0.0) == np.array_equal(guarded[0], _bits(torch.from_numpy(p0)))
        assert all(g.intact() for g in (m, v, p, prev))


# ------------------------------------------------------------------------------------------------------------------------------
# 4. bad arguments
# ------------------------------------------------------------------------------------------------------------------------------
def test_optimism_refuses_bad_arguments():
    lib = _lib()
    n = 1024
    rng = np.random.default_rng(7)
    bufs = {k: Guarded(k, n, rng.standard_normal(n) ** 2 + 1e-3) for k in ("p", "prev", "m", "v")}
    before = {k: _bits(g.raw) for k, g in bufs.items()}
    call = _Call([n], [0.05], 3)
    words = torch.zeros(8, dtype=torch.int32, device=dev())
    good = dict(p=bufs["p"].ptr, prev=bufs["prev"].ptr, m=bufs["m"].ptr, v=bufs["v"].ptr, n=n, seg=call.seg.data_ptr(),
                lr=call.lr.data_ptr(), n_seg=1, b1=0.0, b2=0.99, eps=EPS, omega=1.0, step=call.step.data_ptr(), state=None, st=_stream())
    order = ("p", "prev", "m", "v", "n", "seg", "lr", "n_seg", "b1", "b2", "eps", "omega", "step", "state", "st")
    bad = {"null " + k: {k: None} for k in ("p", "prev", "m", "v", "seg", "lr", "step")}
    bad.update({"n = 0": {"n": 0}, "n < 0": {"n": -4}, "no segment": {"n_seg": 0}, "17 segments": {"n_seg": 17},
                "omega < 0": {"omega": -0.25}, "omega > 1": {"omega": 1.5}, "omega NaN": {"omega": float("nan")}})
    bad.update({k + " + 4 bytes": {k: good[k] + 4, "n": n - 1} for k in ("p", "prev", "m", "v")})
    bad.update({"prev == " + k: {"prev": good[k]} for k in ("p", "m", "v")})
    bad.update({"prev inside " + k: {"prev": good[k] + 16, "n": n - 4} for k in ("p", "m", "v")})
    bad.update({"prev in front of p": {"p": good["prev"] + 16, "n": n - 4}, "step + 1 byte": {"step": good["step"] + 1},
                "step + 2 bytes": {"step": good["step"] + 2}, "state + 1 byte": {"state": words.data_ptr() + 1}})
    for what, change in bad.items():
        args = dict(good, **change)
        assert lib.gim_adam_optimism(*[args[k] for k in order]) != 0, what
        msg = lib.gim_last_error().decode()
        assert "adam_optimism" in msg, (what, msg)
    torch.cuda.synchronize()
    for k, g in bufs.items():
        assert np.array_equal(_bits(g.raw), before[k]), (k, "a refused call wrote")
    for omega in (0.0, 1.0):     # both ends of the closed interval are taken
        assert lib.gim_adam_optimism(*[dict(good, omega=omega)[k] for k in order]) == 0, lib.gim_last_error()
    torch.cuda.synchronize()
    assert all(g.intact() for g in bufs.values())


# ------------------------------------------------------------------------------------------------------------------------------
# 5. FusedAdam
# ------------------------------------------------------------------------------------------------------------------------------
def _host(t):
    return t.detach().double().cpu().contiguous().numpy()


def _read(named):
    return {k: _host(p) for k, p in named.items()}


def _adam_state(opt, named):
    """{name: (exp_avg, exp_avg_sq, step)} on the host, read from state_dict() (torch.optim.Adam's packed format), and
    {name: the learning rate of its group}."""
    sd = opt.state_dict()
    by_param, lrs = {}, {}
    for group, packed in zip(opt.param_groups, sd["param_groups"]):
        for p, idx in zip(group["params"], packed["params"]):
            by_param[p], lrs[p] = sd["state"][idx], packed["lr"]
    out = {k: (_host(by_param[p]["exp_avg"]), _host(by_param[p]["exp_avg_sq"]), int(by_param[p]["step"])) for k, p in named.items()}
    return out, {k: np.float32(lrs[p]) for k, p in named.items()}


def _directions(opt, named):
    """d_t of every parameter, recomputed on the host in fp64 from the optimizer's state, and the learning rates."""
    g0 = opt.param_groups[0]
    state, lrs = _adam_state(opt, named)
    return {k: ref.direction(m, v, g0["betas"][0], g0["betas"][1], g0["eps"], t) for k, (m, v, t) in state.items()}, lrs


def _prev_by_name(opt, named):
    prev = opt.optimism_state()
    return {k: _host(prev[p]) for k, p in named.items()}


def _check_optimistic_step(what, opt, named, p_before, prev_before, omega):
    """p_t = p_{t-1} - lr (d_t + omega (d_t - d_{t-1})) within step_bound, optimism_state() = d_t within direction_bound, and p_t from
    the returned directions; returns (p_t, d_t as the device holds it)."""
    torch.cuda.synchronize()
    d, lrs = _directions(opt, named)
    p_now, prev_now = _read(named), _prev_by_name(opt, named)
    w = float(np.float32(omega))
    worst, moved = [0.0, 0.0], False
    for k in named:
        lr = float(lrs[k])
        want = p_before[k] - lr * (d[k] + w * (d[k] - prev_before[k]))
        worst[0] = max(worst[0], _worst(np.abs(p_now[k] - want), step_bound(p_before[k], want, d[k], prev_before[k], lrs[k], w)))
        worst[1] = max(worst[1], _worst(np.abs(prev_now[k] - d[k]), direction_bound(d[k])))
        moved = moved or float(np.abs(p_now[k] - p_before[k]).max()) > 0.1 * lr
    assert moved, (what, "the step did not move the parameters")
    print("%s: error / bound  p %.3f  prev %.3f" % (what, worst[0], worst[1]))
    assert worst[0] <= 1.0 and worst[1] <= 1.0, (what, worst)
    return p_now, prev_now


def _seeded_grads(named, tag):
    with torch.no_grad():
        for k, p in named.items():
            p.grad.copy_(T(pf.normal("%s/%s" % (tag, k), tuple(p.shape))).float())


def _make_params(tag, shapes):
    named = {}
    for k, sh in shapes.items():
        v = T(pf.normal("%s/init/%s" % (tag, k), sh)).float().to(dev())
        named[k] = torch.nn.Parameter(v.contiguous(memory_format=torch.channels_last) if len(sh) == 4 else v)
    return named


def test_fused_adam_steps_optimistically():
    from optimalstrategiesagainstgenerativeattacks_amd.optim import FusedAdam
    tag, omega, decay, betas = "oadam/opt", 1.0, 0.5, (0.5, 0.9)
    named = _make_params(tag, {"a": (7,), "b": (64,), "c": (100,), "w": (4, 5, 3, 3)})     # padded slots exist
    opt = FusedAdam([{"params": [named["a"], named["b"]], "lr": 0.05}, {"params": [named["c"], named["w"]], "lr": 0.0125}], lr=0.05,
                    betas=betas)
    opt.enable_optimism(omega)
    opt.enable_averaging(decay)
    assert opt.optimism == omega
    opt.zero_grad()
    opt.prime_optimism()      # no applied step: nothing to record
    prev = _prev_by_name(opt, named)
    assert all(v.shape == tuple(named[k].shape) and not v.any() for k, v in prev.items()), "prev starts as zeros"
    p_now = _read(named)
    avg = {k: v.copy() for k, v in p_now.items()}       # the average starts as the weights
    d_e = np.float64(np.float32(decay)), np.float64(np.float32(1.0) - np.float32(decay))
    big = 0.0

    def one_step(t, p_now, prev):
        opt.zero_grad()
        _seeded_grads(named, "%s/g%d" % (tag, t))
        opt.step()
        return _check_optimistic_step("step %d" % t, opt, named, p_now, prev, omega)

    for t in range(3):
        if t == 2:      # the parameters move to new storage: the optimizer rebuilds its buffers and prev goes with them
            old = opt.flat_prev.data_ptr()
            with torch.no_grad():
                for p in named.values():
                    p.data = p.data.clone()
            opt.zero_grad()
            assert opt.flat_prev.data_ptr() != old, "the optimizer did not rebuild"
            moved = _prev_by_name(opt, named)
            assert all(np.array_equal(moved[k], prev[k]) for k in named), "the rebuild changed prev"
        p_now, prev = one_step(t, p_now, prev)
        # the average follows the CORRECTED weights: behind a launch order Adam, average, correction it would hold
        # d avg + e (p + lr omega (d_t - d_{t-1})), lr |d_t - d_{t-1}| / 2 away
        got = opt.average_state()
        for k, p in named.items():
            avg[k] = d_e[0] * avg[k] + d_e[1] * p_now[k]
            big = max(big, float(np.abs(p_now[k]).max()), float(np.abs(avg[k]).max()))
            bound = (t + 1) * 4 * U * 2 * big              # test_gpu_weight_average.py: T updates, each 4 u (|avg| + |p|)
            err = float(np.abs(_host(got[p]) - avg[k]).max())
            assert err <= bound, (t, k, "the average did not see the corrected weights", err, bound)
    mask = torch.zeros(opt.flat_prev.numel(), dtype=torch.bool, device=dev())
    for o, n in opt._offsets.values():
        mask[o:o + n] = True
    assert int((~mask).sum()) > 0 and not bool(opt.flat_prev[~mask].any()) and not bool(opt.flat_p[~mask].any()), "padding stays zeros"
    assert set(opt.state_dict()["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}, "state_dict() keeps torch.optim.Adam's format"

    # load_optimism / prime_optimism
    opt.load_optimism({named["b"]: torch.full((64,), 0.25)})
    now = _prev_by_name(opt, named)
    assert (now["b"] == 0.25).all() and np.array_equal(now["a"], prev["a"])
    p_bits = {k: _bits(p) for k, p in named.items()}
    opt.prime_optimism()
    torch.cuda.synchronize()
    primed = _prev_by_name(opt, named)
    assert all(np.array_equal(primed[k], prev[k]) for k in named), "priming records the d of the current state"
    assert all(np.array_equal(_bits(p), p_bits[k]) for k, p in named.items()), "priming touched the parameters"

    # inside averaged_weights() the parameters hold the averages: nothing of this may run
    with opt.averaged_weights():
        for call in (opt.optimism_state, opt.prime_optimism, lambda: opt.load_optimism({}), lambda: opt.enable_optimism(0.5),
                     opt.disable_optimism):
            with pytest.raises(RuntimeError, match="averaged_weights"):
                call()
    assert opt.optimism == omega
    opt.disable_optimism()
    assert opt.optimism is None and opt.flat_prev is None
    opt.zero_grad()
    _seeded_grads(named, tag + "/g3")
    opt.step()       # and the optimizer steps plainly again
    opt.enable_optimism(0.5)      # after the build: allocated at once, zeros
    assert opt.flat_prev is not None and not bool(opt.flat_prev.any())


# ------------------------------------------------------------------------------------------------------------------------------
# 6. a step the loss scaler skips
# ------------------------------------------------------------------------------------------------------------------------------
def test_skipped_step_is_a_skipped_correction():
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    from optimalstrategiesagainstgenerativeattacks_amd.optim import FusedAdam
    tag, omega = "oadam/skip", 1.0
    prev_path = ops.set_matrix_path("fp16")
    prev_scale = ops.set_loss_scale("dynamic")
    try:
        w0 = (T(pf.normal(tag + "/w", (64, 32, 3, 3))) / np.sqrt(288.0)).float().to(dev())
        named = {"w": torch.nn.Parameter(w0.contiguous(memory_format=torch.channels_last))}
        w = named["w"]
        opt = FusedAdam([w], lr=0.05, betas=(0.0, 0.99))
        opt.enable_optimism(omega)
        opt.zero_grad()
        sc = opt.dynamic_scaler()
        assert sc is not None and opt.loss_scaler is sc
        scale = sc.state()["scale"]

        def grads(t):      # the bucket holds gradients of scale * loss
            _seeded_grads(named, "%s/g%d" % (tag, t))
            opt.flat_g.mul_(scale)

        p_start = _read(named)
        grads(0)
        opt.step()
        p_now, prev = _check_optimistic_step("clean step", opt, named, p_start, {"w": np.zeros(tuple(w.shape))}, omega)
        assert float(np.abs(prev["w"]).mean()) > 0.5, "prev is not of order 1"
        before = {k: _bits(t) for k, t in (("p", w), ("m", opt.flat_m), ("v", opt.flat_v), ("prev", opt.flat_prev))}
        opt.zero_grad()
        grads(1)
        opt.flat_g[opt._offsets[w][0] + 1] = float("inf")
        opt.step()
        st = sc.state()
        assert st["skipped"] == 1 and st["last_overflow"], "the step was not skipped"
        after = {k: _bits(t) for k, t in (("p", w), ("m", opt.flat_m), ("v", opt.flat_v), ("prev", opt.flat_prev))}
        for k in before:
            assert np.array_equal(before[k], after[k]), (k, "a skipped step changed it")
        assert _adam_state(opt, named)[0]["w"][2] == 1, "a skipped step counted"

        scale = st["scale"]
        opt.zero_grad()
        grads(2)
        opt.step()
        assert sc.state()["skipped"] == 1 and _adam_state(opt, named)[0]["w"][2] == 2
        _check_optimistic_step("clean step after the skipped one", opt, named, p_now, prev, omega)
    finally:
        ops.set_loss_scale(prev_scale)
        ops.set_matrix_path(prev_path)


# ------------------------------------------------------------------------------------------------------------------------------
# 7. the bilinear game on the device
# ------------------------------------------------------------------------------------------------------------------------------
def _device_game(omega, steps=1000):
    from optimalstrategiesagainstgenerativeattacks_amd.optim import FusedAdam
    x0, y0 = ref.bilinear_start(0)
    x, y = (torch.nn.Parameter(torch.from_numpy(a).float().to(dev())) for a in (x0, y0))
    opts = [FusedAdam([q], lr=3e-2, betas=(0.0, 0.99), eps=1e-8) for q in (x, y)]
    for opt in opts:
        if omega:
            opt.enable_optimism(omega)
        opt.zero_grad()
    with torch.no_grad():
        for _ in range(steps):
            x.grad.copy_(y)              # both gradients from the pre-step iterate
            y.grad.copy_(x).neg_()
            for opt in opts:
                opt.step()
    torch.cuda.synchronize()
    start = np.sqrt((x0 ** 2).sum() + (y0 ** 2).sum())
    return float(np.sqrt((_host(x) ** 2).sum() + (_host(y) ** 2).sum()) / start)


def test_bilinear_game_on_the_device():
    """The conditions of test_optimism_host.test_bilinear_game_in_fp64, on FusedAdam in fp32 (fp64 over seeds 0-19: 0.575-0.678 and
    0.055-0.123).  Conditions on where the game ends, not a comparison of trajectories."""
    plain, optimistic = _device_game(None), _device_game(1.0)
    print("bilinear game on the device, seed 0: final / start distance %.4f (plain)  %.4f (omega 1)" % (plain, optimistic))
    assert plain >= 0.45, plain
    assert optimistic <= 0.25, optimistic


# ------------------------------------------------------------------------------------------------------------------------------
# 8. the trainers
# ------------------------------------------------------------------------------------------------------------------------------
CFG = "16_1_32"
B, M, N, K, C, S, D = 2, 1, 3, 4, 1, 16, 32
LR = 1e-2


@pytest.fixture()
def det():
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    prev = ops.set_deterministic(True)
    yield ops
    ops.set_deterministic(prev)


def _img_trainer(outdir, tag, **kw):
    import optimalstrategiesagainstgenerativeattacks_amd as G
    keys = load_keys(CFG)
    au, im = G.get_au(S, C, D), G.get_im(S, C, D)
    au.load_state_dict(filled_sd(keys["au"], tag + "/au/", torch.float32))
    im.load_state_dict(filled_sd(keys["im"], tag + "/im/", torch.float32))
    return G.GIMImgTrainer(outdir, M, N, K, au.to(dev()), im.to(dev()), LR, LR, LR / 4, reg_param=0.0, **kw)


def _agents(tr):
    return {"im": (tr.impersonator, tr.impersonator_opt), "au": (tr.authenticator, tr.authenticator_opt)}


def _named(tr):
    return {a: dict(mod.named_parameters()) for a, (mod, _) in _agents(tr).items()}


def _step(tr, it, tag):
    import optimalstrategiesagainstgenerativeattacks_amd as G
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    ep = [t.float().to(dev()) for t in episode("%s/%d" % (tag, it), B, M, N, K, C, S, D)]
    tr.do_global_step()
    out = G.gim_step(G.DataParallelMock(tr), *ep[:3], z=ep[3])
    ops.join_lanes()
    torch.cuda.synchronize()
    return out


def _state_bits(tr):
    """Everything a resumed trainer must reproduce: parameters and buffers of both agents, bit patterns."""
    return {a + "." + k: _bits(v.float()) for a, (mod, _) in _agents(tr).items() for k, v in mod.state_dict().items()}


def _ckpt(tr):
    tr.save(epoch=0)
    return os.path.join(tr.checkpoint_dir, "model_{:08}.pt".format(tr.global_step))


def test_trainer_steps_optimistically(det):
    tag = "oadam/tr"
    with tempfile.TemporaryDirectory() as td:
        plain = _img_trainer(os.path.join(td, "plain"), tag)
        opt = _img_trainer(os.path.join(td, "opt"), tag, im_optimism=1.0, au_optimism=1.0)
        assert plain.impersonator_opt.optimism is None and opt.impersonator_opt.optimism == 1.0 and opt.authenticator_opt.optimism == 1.0
        p0 = {a: _read(nm) for a, nm in _named(plain).items()}
        assert all(np.array_equal(p0[a][k], v) for a, nm in _named(opt).items() for k, v in _read(nm).items())

        # ---- the first step: same gradients, prev = 0, so the optimistic trainer moves twice as far
        (gi_p, di_p), (gi_o, di_o) = _step(plain, 0, tag), _step(opt, 0, tag)
        for what, a, b in (("g loss", gi_p[0], gi_o[0]), ("fake", gi_p[1], gi_o[1]), ("g logits", gi_p[2], gi_o[2]),
                           ("d loss", di_p[0], di_o[0]), ("d out on real", di_p[4], di_o[4]), ("d out on fake", di_p[5], di_o[5])):
            assert torch.equal(a, b), (what, "the first step's outputs differ between the two trainers")
        p1_plain, p1_opt = ({a: _read(nm) for a, nm in _named(tr).items()} for tr in (plain, opt))
        worst, moved = 0.0, 0
        for a in p0:
            for k in p0[a]:
                lhs, rhs = p1_opt[a][k] - p0[a][k], 2 * (p1_plain[a][k] - p0[a][k])
                # beta1 = 0, t = 1: Adam's direction is d^ itself (docstring, A), |d| < 1, and with a = fl(lr d^) the two stores give
                # |lhs - rhs| <= u (|p_plain| + |p_opt| + 2 |a|), |a| <= lr |d^|
                bound = U * (np.abs(p1_plain[a][k]) + np.abs(p1_opt[a][k]) + 2 * 1.01 * LR)     # 1.01: |d^| <= 1 + O(u)
                worst = max(worst, _worst(np.abs(lhs - rhs), bound))
                moved += int((np.abs(rhs) > 0.5 * LR / 4).sum())
        print("first step, p_opt - p_0 against 2 (p_plain - p_0): error / bound %.3f over %d moved elements" % (worst, moved))
        assert worst <= 1.0 and moved > 1000, (worst, moved)

        # ---- checkpoints: the entry, and a resumed trainer continues bit for bit
        path_opt, path_plain = _ckpt(opt), _ckpt(plain)
        payload = torch.load(path_opt, map_location="cpu", weights_only=False)
        assert set(payload) == set(opt.CHECKPOINT_KEYS) | {"global_step", "last_epoch", "optimism"}
        assert set(payload["optimism"]) == {"impersonator", "authenticator"}
        assert payload["optimism"]["impersonator"]["omega"] == 1.0
        assert set(payload["optimism"]["impersonator"]["state"]) == set(_named(opt)["im"])
        assert set(payload["optimism"]["authenticator"]["state"]) == set(_named(opt)["au"])
        assert set(torch.load(path_plain, map_location="cpu", weights_only=False)) == set(plain.CHECKPOINT_KEYS) | {"global_step", "last_epoch"}

        resumed = _img_trainer(os.path.join(td, "resumed"), tag + "/other", im_optimism=1.0, au_optimism=1.0)
        resumed.resume_from_ckpt(path_opt)
        for a, (_, o) in _agents(resumed).items():
            want = _prev_by_name(_agents(opt)[a][1], _named(opt)[a])
            got = _prev_by_name(o, _named(resumed)[a])
            assert all(np.array_equal(got[k], want[k]) for k in want), (a, "resumed prev")

        # ---- an optimistic trainer resumed from the plain file: prev is primed with the d of the loaded Adam state
        primed = _img_trainer(os.path.join(td, "primed"), tag + "/other", im_optimism=1.0, au_optimism=1.0)
        primed.resume_from_ckpt(path_plain)
        d1 = {}
        for a, (_, o) in _agents(primed).items():
            nm = _named(primed)[a]
            d1[a], _ = _directions(o, nm)
            got = _prev_by_name(o, nm)
            r = max(_worst(np.abs(got[k] - d1[a][k]), direction_bound(d1[a][k])) for k in nm)
            print("primed %s: prev against the host's d, error / bound %.3f" % (a, r))
            assert r <= 1.0, (a, r)
            assert max(float(np.abs(v).max()) for v in got.values()) > 0.5, (a, "prev was not primed")
            loaded = _read(nm)
            assert all(np.array_equal(loaded[k], p1_plain[a][k]) for k in nm), (a, "priming or loading moved the parameters")

        # ---- the second step
        _step(opt, 1, tag)
        _step(resumed, 1, tag)
        s_opt, s_res = _state_bits(opt), _state_bits(resumed)
        diff = [k for k in s_opt if not np.array_equal(s_opt[k], s_res[k])]
        assert not diff, ("the resumed trainer left the uninterrupted one", diff[:5])

        # The primed trainer and the plain one start the step from the same weights, moments and spectral-norm vectors, so their
        # gradients and d_2 are bit-equal and the primed trainer's step is the plain one plus the correction against the PRIMED
        # direction: p_primed = p_plain - lr omega (d_2 - d_1).  It is a plain Adam step up to the change of direction - a prev of
        # zeros would put lr d_2 there, a doubled step.
        _step(plain, 1, tag)
        _step(primed, 1, tag)
        worst = doubled = 0.0
        for a, (_, o) in _agents(primed).items():
            nm = _named(primed)[a]
            d2, lrs = _directions(o, nm)
            p_primed, p_plain = _read(nm), _read(_named(plain)[a])
            for k in nm:
                want = ref.correction(p_plain[k], d1[a][k], d2[k], lrs[k], 1.0)
                bound = correction_bound(want, d2[k], d1[a][k], lrs[k], 1.0) + float(lrs[k]) * direction_bound(d1[a][k])   # d_1 on the host
                worst = max(worst, _worst(np.abs(p_primed[k] - want), bound))
                doubled = max(doubled, _worst(np.abs(p_primed[k] - ref.correction(p_plain[k], 0.0 * d2[k], d2[k], lrs[k], 1.0)), bound))
        print("primed trainer's next step against the plain trainer's: error / bound %.3f (a doubled step: %.3g)" % (worst, doubled))
        assert worst <= 1.0 and doubled > 1e3, (worst, doubled)


def test_gaussian_trainer_steps_optimistically():
    import optimalstrategiesagainstgenerativeattacks_amd as G
    from optimalstrategiesagainstgenerativeattacks_amd import gim_gaussian_models as ggm
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    tag = "oadam/gauss"
    meta = load_json("gaussian.json")
    c = meta["config"]
    au, im = ggm.get_au(c["d"]), ggm.get_im(c["d"])
    au.load_state_dict(filled_sd(meta["keys"]["au"], tag + "/au/", torch.float32))
    im.load_state_dict(filled_sd(meta["keys"]["im"], tag + "/im/", torch.float32))
    omegas = {"im": 1.0, "au": 0.5}
    with tempfile.TemporaryDirectory() as td:
        tr = G.GIMGaussianTrainer(td, c["m"], c["n"], c["k"], au.to(dev()), im.to(dev()), au_lr=c["au_lr"], im_lr=c["im_lr"],
                                  im_optimism=omegas["im"], au_optimism=omegas["au"])
    for _, opt in _agents(tr).values():
        opt.zero_grad()
    named = _named(tr)
    p_now = {a: _read(named[a]) for a in named}
    prev = {a: {k: np.zeros_like(v) for k, v in p_now[a].items()} for a in named}
    for it in range(2):
        mu = pf.normal("%s/it%d/mu" % (tag, it), (c["B"], 1, c["d"]))
        smp = lambda nm, t: T(mu + c["sigma"] * pf.normal("%s/it%d/%s" % (tag, it, nm), (c["B"], t, c["d"]))).float().to(dev())  # noqa: E731
        z = T(pf.normal("%s/it%d/z" % (tag, it), (c["B"], c["n"], c["d"]))).float().to(dev())
        tr.do_global_step()
        G.gim_step(G.DataParallelMock(tr), smp("leaked", c["m"]), smp("real", c["n"]), smp("si", c["k"]), z=z)
        ops.join_lanes()
        for a, (_, opt) in _agents(tr).items():
            p_now[a], prev[a] = _check_optimistic_step("gaussian %s step %d" % (a, it), opt, named[a], p_now[a], prev[a], omegas[a])
