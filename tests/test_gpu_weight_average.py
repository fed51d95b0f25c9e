"""Averaged agents on the GPU: the two kernels of csrc/ema.hip at the C ABI, FusedAdam's average (build, recurrence, re-home,
exchange, skipped step), the cached weight copies across the exchange, and the trainer (recurrence over gim_steps, evaluation on
the averaged weights against the oracle, checkpoints, authentication_eval).

Bounds.  avg' = fl(fl(d a) + fl(e p)) with d = float32(decay), e = fl(1 - d): three roundings (two with a fused multiply-add), each
at most 2^-24 relative to a quantity no larger than |a| + |p|, against an fp64 reference built from the same d and e:
4 * 2^-24 * (|a| + |p|) per update.  Over T updates the errors of earlier updates are carried with a factor d < 1 and each update
adds at most the one-update bound at the largest magnitude seen, M: T * 4 * 2^-24 * 2 M.  Derived, not measured."""
import ctypes
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import gim_oracle as go
from oracle import portable_fill as pf
from tests.helpers import Guarded, T, episode, load_keys, relerr

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
GRID_PASS = 4096 * 256 * 4      # floats one pass of the capped grid covers (adam.hip's launch shape)
SIZES = [1, 3, 4, 5, 255, 1024, 1025, GRID_PASS + 1029]   # the last: the grid-stride loop runs twice, then a tail of one
DECAYS = [0.0, 0.5, 0.999]
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


def _d_e(decay):
    d = np.float32(decay)
    return d, np.float32(np.float32(1.0) - d)


def _ema_ref(avg, p, decay):
    d, e = _d_e(decay)
    return np.float64(d) * np.asarray(avg, np.float64) + np.float64(e) * np.asarray(p, np.float64)


# ------------------------------------------------------------------------------------------------------------------------------
# 1. gim_ema_update at the C ABI
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_ema_update_kernel(n):
    lib = _lib()
    rng = np.random.default_rng(1000 + n % 9973)
    a0 = rng.standard_normal(n).astype(np.float32)
    p0 = rng.standard_normal(n).astype(np.float32)
    avg, p = Guarded("avg", n, a0), Guarded("p", n, p0)
    p_bits = _bits(p.t)
    for decay in DECAYS:
        avg.fill(a0)
        assert lib.gim_ema_update(avg.ptr, p.ptr, n, decay, None, _stream()) == 0, lib.gim_last_error()
        torch.cuda.synchronize()
        got = avg.np()
        ref = _ema_ref(a0, p0, decay)
        bound = 4 * U * (np.abs(a0.astype(np.float64)) + np.abs(p0.astype(np.float64)))
        ratio = float((np.abs(got - ref) / bound).max())
        print("ema_update n %d decay %g: worst error / bound %.3f" % (n, decay, ratio))
        assert ratio <= 1.0, (n, decay, ratio)
        if decay == 0.0:
            assert np.array_equal(_bits(avg.t), p_bits), "decay 0: avg is p bit for bit"
        assert avg.intact() and p.intact(), "guard bands"
        assert np.array_equal(_bits(p.t), p_bits), "p changed"

    # behind a loss scaler: the last word of its state decides; the other seven are only read
    words_host = np.array([0x45800000, 0x39800000, 2000, 5, 0, 3, 0x3F800000, 1], dtype=np.int32)
    words = torch.from_numpy(words_host).to(dev())
    avg.fill(a0)
    before = _bits(avg.t)
    assert lib.gim_ema_update(avg.ptr, p.ptr, n, 0.5, words.data_ptr(), _stream()) == 0, lib.gim_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(avg.t), before), "a skipped step moved the average"
    assert np.array_equal(words.cpu().numpy(), words_host)
    words_host[SC_LAST_OVERFLOW] = 0
    words.copy_(torch.from_numpy(words_host))
    assert lib.gim_ema_update(avg.ptr, p.ptr, n, 0.5, words.data_ptr(), _stream()) == 0, lib.gim_last_error()
    torch.cuda.synchronize()
    guarded = _bits(avg.t)
    assert np.array_equal(words.cpu().numpy(), words_host)
    avg.fill(a0)
    assert lib.gim_ema_update(avg.ptr, p.ptr, n, 0.5, None, _stream()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(guarded, _bits(avg.t)), "the guarded update is the plain one when the step was applied"
    assert not np.array_equal(guarded, before)
    assert avg.intact() and p.intact()


def test_ema_update_refuses_bad_arguments():
    lib = _lib()
    n = 1024
    rng = np.random.default_rng(7)
    avg, p = Guarded("avg", n, rng.standard_normal(n)), Guarded("p", n, rng.standard_normal(n))
    a_bits, p_bits = _bits(avg.raw), _bits(p.raw)
    st = _stream()
    bad = {"null avg": (None, p.ptr, n, 0.5, None, st), "null p": (avg.ptr, None, n, 0.5, None, st),
           "n = 0": (avg.ptr, p.ptr, 0, 0.5, None, st), "decay = 1": (avg.ptr, p.ptr, n, 1.0, None, st),
           "decay NaN": (avg.ptr, p.ptr, n, float("nan"), None, st), "decay < 0": (avg.ptr, p.ptr, n, -0.25, None, st),
           "avg + 1": (avg.ptr + 4, p.ptr, n - 1, 0.5, None, st), "avg == p": (avg.ptr, avg.ptr, n, 0.5, None, st),
           "state + 1 byte": (avg.ptr, p.ptr, n, 0.5, p.ptr + 1, st)}
    for what, args in bad.items():
        assert lib.gim_ema_update(*args) != 0, what
        msg = lib.gim_last_error().decode()
        assert "ema_update" in msg, (what, msg)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(avg.raw), a_bits) and np.array_equal(_bits(p.raw), p_bits), "a refused call wrote"


# ------------------------------------------------------------------------------------------------------------------------------
# 2. gim_buffer_exchange
# ------------------------------------------------------------------------------------------------------------------------------
# quiet and signalling NaNs with payloads, +-0, +-inf, the smallest and the largest denormal
SPECIALS = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF],
                    dtype=np.uint32).view(np.int32)


def _patterns(rng, n):
    bits = rng.integers(-2 ** 31, 2 ** 31, size=n, dtype=np.int64).astype(np.int32)
    k = min(n, len(SPECIALS))
    bits[:k] = SPECIALS[:k]
    bits[n - k:] = SPECIALS[:k][::-1]      # the scalar tail sees them too
    return bits


def _set_bits(g, bits):
    g.t.view(torch.int32).copy_(torch.from_numpy(bits).to(dev()))


@pytest.mark.parametrize("n", SIZES)
def test_buffer_exchange_kernel(n):
    lib = _lib()
    rng = np.random.default_rng(2000 + n % 9973)
    a_bits, b_bits = _patterns(rng, n), _patterns(rng, n)[::-1].copy()
    a, b = Guarded("a", n), Guarded("b", n)
    _set_bits(a, a_bits)
    _set_bits(b, b_bits)
    assert lib.gim_buffer_exchange(a.ptr, b.ptr, n, _stream()) == 0, lib.gim_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(a.t), b_bits) and np.array_equal(_bits(b.t), a_bits), "one call swaps the bit patterns"
    assert a.intact() and b.intact()
    assert lib.gim_buffer_exchange(a.ptr, b.ptr, n, _stream()) == 0, lib.gim_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(a.t), a_bits) and np.array_equal(_bits(b.t), b_bits), "two calls are the identity"
    assert a.intact() and b.intact()
    assert lib.gim_buffer_exchange(a.ptr, a.ptr, n, _stream()) != 0, "a == b"
    assert "buffer_exchange" in lib.gim_last_error().decode()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(a.t), a_bits)


def test_buffer_exchange_refuses_bad_arguments():
    lib = _lib()
    n = 1024
    big = Guarded("big", 2 * n, np.arange(2 * n))
    other = Guarded("other", n, np.arange(n))
    before = _bits(big.raw), _bits(other.raw)
    st = _stream()
    bad = {"overlap, b behind a": (big.ptr, big.ptr + 16, n, st), "overlap, a behind b": (big.ptr + 4 * (n - 4), big.ptr, n, st),
           "null a": (None, other.ptr, n, st), "null b": (other.ptr, None, n, st), "n = 0": (big.ptr, other.ptr, 0, st),
           "a + 1": (big.ptr + 4, other.ptr, n, st)}
    for what, args in bad.items():
        assert lib.gim_buffer_exchange(*args) != 0, what
        assert "buffer_exchange" in lib.gim_last_error().decode(), what
    torch.cuda.synchronize()
    assert np.array_equal(_bits(big.raw), before[0]) and np.array_equal(_bits(other.raw), before[1]), "a refused call wrote"
    assert lib.gim_buffer_exchange(big.ptr, big.ptr + 4 * n, n, st) == 0, "adjacent ranges do not overlap"
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------------------
# 3. FusedAdam
# ------------------------------------------------------------------------------------------------------------------------------
LR, BETAS, DECAY = 0.05, (0.0, 0.99), 0.5


class _Recurrence:
    """The fp64 recurrence avg <- d avg + e p on values read back from the device, and the largest magnitude it has seen."""

    def __init__(self, start, decay):
        self.d, self.e = (np.float64(x) for x in _d_e(decay))
        self.avg = {k: v.clone() for k, v in start.items()}
        self.big = max(float(v.abs().max()) for v in start.values())
        self.steps = 0

    def update(self, p):
        for k, v in p.items():
            self.avg[k] = self.d * self.avg[k] + self.e * v
            self.big = max(self.big, float(v.abs().max()))
        self.steps += 1

    def bound(self):
        return self.steps * 4 * U * self.big * 2

    def check(self, got, what):
        worst = max(float((got[k] - self.avg[k]).abs().max()) for k in self.avg)
        print("%s: %d updates, worst error %.3e, bound %.3e" % (what, self.steps, worst, self.bound()))
        assert worst <= self.bound(), (what, worst, self.bound())


def _host(t):
    return t.detach().double().cpu().contiguous()


def _read(named):
    return {k: _host(p) for k, p in named.items()}


def _avg_by_name(opt, named):
    avg = opt.average_state()
    return {k: _host(avg[p]) for k, p in named.items()}


def _seeded_grads(named, tag):
    with torch.no_grad():
        for k, p in named.items():
            p.grad.copy_(T(pf.normal("%s/%s" % (tag, k), tuple(p.shape))).float())


def test_fused_adam_keeps_the_average():
    from optimalstrategiesagainstgenerativeattacks_amd.optim import FusedAdam, weights_epoch
    tag = "wavg/opt"
    shapes = {"a": (7,), "b": (64,), "c": (100,), "w": (4, 5, 3, 3)}     # 7, 64, 100 and 4*3*3*5 elements: padded slots exist
    named = {}
    for k, sh in shapes.items():
        v = T(pf.normal("%s/init/%s" % (tag, k), sh)).float().to(dev())
        named[k] = torch.nn.Parameter(v.contiguous(memory_format=torch.channels_last) if len(sh) == 4 else v)
    opt = FusedAdam([{"params": [named["a"], named["b"]]}, {"params": [named["c"], named["w"]]}], lr=LR, betas=BETAS)
    opt.enable_averaging(DECAY)
    assert opt.averaging == DECAY
    opt.zero_grad()
    avg = opt.average_state()
    for k, p in named.items():
        assert avg[p].shape == p.shape and torch.equal(avg[p], p.detach()), (k, "at enable the average is the weights")
    start = _read(named)
    rec = _Recurrence(start, DECAY)
    for t in range(3):
        opt.zero_grad()
        _seeded_grads(named, "%s/g%d" % (tag, t))
        opt.step()
        torch.cuda.synchronize()
        rec.update(_read(named))
        rec.check(_avg_by_name(opt, named), "step %d" % t)
    mask = torch.zeros(opt.flat_avg.numel(), dtype=torch.bool, device=dev())
    for o, n in opt._offsets.values():
        mask[o:o + n] = True
    assert int((~mask).sum()) > 0 and not bool(opt.flat_avg[~mask].any()), "padding of flat_avg is zeros"
    assert not bool(opt.flat_p[~mask].any())
    got = _avg_by_name(opt, named)
    for k in named:
        assert float((got[k] - start[k]).abs().max()) > 100 * rec.bound(), (k, "the average did not move")

    # the parameters move to new storage: the optimizer rebuilds its buffers and the average goes with them
    old_avg_ptr = opt.flat_avg.data_ptr()
    with torch.no_grad():
        for p in named.values():
            p.data = p.data.clone()
    opt.zero_grad()
    assert opt.flat_avg.data_ptr() != old_avg_ptr, "the optimizer did not rebuild"
    after_move = _avg_by_name(opt, named)
    for k in named:
        assert torch.equal(after_move[k], got[k]), (k, "the rebuild changed the average")
    _seeded_grads(named, tag + "/g3")
    opt.step()
    torch.cuda.synchronize()
    rec.update(_read(named))
    rec.check(_avg_by_name(opt, named), "step after the move")
    assert not bool(opt.flat_avg[~mask].any())

    # averaged_weights(): the parameters hold the averages inside, the live values outside
    saved_avg = {k: opt.average_state()[p].detach().clone() for k, p in named.items()}
    saved_live = {k: p.detach().clone() for k, p in named.items()}
    for k in named:
        assert float((saved_avg[k] - saved_live[k]).abs().max()) > 100 * rec.bound(), (k, "average and weights coincide")
    e0 = {k: weights_epoch(p) for k, p in named.items()}
    ptrs = {k: p.data_ptr() for k, p in named.items()}
    with opt.averaged_weights():
        for k, p in named.items():
            assert torch.equal(p.detach(), saved_avg[k]), (k, "inside: the average")
            assert weights_epoch(p) > e0[k], k
        e1 = {k: weights_epoch(p) for k, p in named.items()}
        for call in (opt.step, opt.zero_grad, lambda: opt.averaged_weights().__enter__()):
            with pytest.raises(RuntimeError):
                call()
    for k, p in named.items():
        assert torch.equal(p.detach(), saved_live[k]), (k, "outside: the live weights")
        assert torch.equal(opt.average_state()[p], saved_avg[k]), k
        assert weights_epoch(p) > e1[k] and p.data_ptr() == ptrs[k], k
    with pytest.raises(KeyError):
        with opt.averaged_weights():
            raise KeyError("from the body")
    for k, p in named.items():
        assert torch.equal(p.detach(), saved_live[k]), (k, "an exception inside still restores")
    opt.zero_grad()      # and the optimizer works again
    opt.disable_averaging()
    assert opt.averaging is None and opt.flat_avg is None


# ------------------------------------------------------------------------------------------------------------------------------
# 4. a step the loss scaler skips
# ------------------------------------------------------------------------------------------------------------------------------
def test_skipped_step_leaves_the_average_alone():
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    from optimalstrategiesagainstgenerativeattacks_amd.optim import FusedAdam
    tag = "wavg/skip"
    prev_path = ops.set_matrix_path("fp16")
    prev_scale = ops.set_loss_scale("dynamic")
    try:
        w0 = (T(pf.normal(tag + "/w", (64, 32, 3, 3))) / np.sqrt(288.0)).float().to(dev())
        w = torch.nn.Parameter(w0.contiguous(memory_format=torch.channels_last))
        named = {"w": w}
        opt = FusedAdam([w], lr=LR, betas=BETAS)
        opt.enable_averaging(DECAY)
        opt.zero_grad()
        sc = opt.dynamic_scaler()
        assert sc is not None and opt.loss_scaler is sc
        # an average that is NOT the weights: an update that ran after all would move every element by 0.5
        opt.load_average({w: w.detach() + 1.0})
        before_avg, before_w = _bits(opt.average_state()[w]), _bits(w)
        _seeded_grads(named, tag + "/g0")
        opt.flat_g[opt._offsets[w][0] + 1] = float("inf")
        opt.step()
        assert sc.state()["skipped"] == 1, "the step was not skipped"
        assert np.array_equal(_bits(w), before_w), "a skipped step moved the parameter"
        assert np.array_equal(_bits(opt.average_state()[w]), before_avg), "a skipped step moved the average"

        rec = _Recurrence(_avg_by_name(opt, named), DECAY)
        opt.zero_grad()
        _seeded_grads(named, tag + "/g1")
        opt.step()
        assert sc.state()["skipped"] == 1
        now = _read(named)
        assert float((now["w"] - _host(w0)).abs().mean()) > 0.5 * LR, "the clean step did not move the weights"
        rec.update(now)
        rec.check(_avg_by_name(opt, named), "clean step after the skipped one")
    finally:
        ops.set_loss_scale(prev_scale)
        ops.set_matrix_path(prev_path)


# ------------------------------------------------------------------------------------------------------------------------------
# 5. the cached weight copies follow the exchange
# ------------------------------------------------------------------------------------------------------------------------------
TOL = 3e-5


def _cache_cases():
    from tests.test_gpu_weight_cache import Case
    return [Case("image", "op", 1, 3, 16, 3, 8, 0.2, False, 0, False, False, TOL, [(3, "rows"), (3, 4)], "rows", ("xfold", 4), "queued_rows"),
            Case("pooled_image", "sn", 1, 3, 16, 3, 8, 0.2, True, 0, False, False, TOL, [(4, "fold"), (4, 0)], "plain", ("t", 0), "queued")]


def _fwd_reference(c, x, w, b, uv):
    """fp64 forward of the unfused form on the CPU; sn: sigma = u^T W v with the stored vectors (eval mode, no power iteration)."""
    wn = w
    if uv is not None:
        wn = go.sn_weight({"weight_orig": w, "weight_u": uv[0].clone(), "weight_v": uv[1].clone()}, "", False)
    y = F.conv2d(F.leaky_relu(x, c.slope), wn, None, padding=(c.K - 1) // 2)
    if c.pool:
        y = F.avg_pool2d(y, 2)
    return y + b.view(1, -1, 1, 1)


@pytest.mark.parametrize("name", ["image", "pooled_image"])
def test_cached_weight_copies_follow_the_exchange(name):
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    from optimalstrategiesagainstgenerativeattacks_amd.optim import FusedAdam
    from tests.test_gpu_weight_cache import _Layer, nchw, nhwc
    c = [cc for cc in _cache_cases() if cc.name == name][0]
    tag = "wavg/cache/" + name
    L = _Layer(ops, c, tag)
    L.opt = FusedAdam(L.params(), lr=LR, betas=BETAS)
    L.opt.enable_averaging(DECAY)
    L.opt.zero_grad()
    L.run(L.inputs(tag + "/1"))      # forward + backward on the live weights: the slots are warm, the bucket holds gradients
    st = L.slots_state()
    assert all(present and not stale for present, stale in st), (c.slots, st)
    L.opt.step()                     # the weights move by ~lr, the average by half of that
    torch.cuda.synchronize()
    for m in L.mods:
        m.eval()
    uv = L.uv()[0]
    w, b = L.ws[0], L.bs[0]
    avg = L.opt.average_state()
    w_avg, b_avg, w_live, b_live = _host(avg[w]), _host(avg[b]), _host(w), _host(b)
    x = T(pf.normal(tag + "/x", (2, c.Cin, c.H, c.H)))

    def forward():
        with torch.no_grad():
            if c.kind == "sn":
                y = L.mods[0](nhwc(x), ups=c.ups, pre_slope=c.slope, pool=c.pool)
            else:
                y = ops.conv2d(nhwc(x), w, b, None, *L.sigma1, c.ups, c.slope, pool=c.pool)
        return nchw(y)
    ref_avg, ref_live = _fwd_reference(c, x, w_avg, b_avg, uv), _fwd_reference(c, x, w_live, b_live, uv)
    assert relerr(ref_avg, ref_live) >= 30 * TOL, ("a stale copy would pass", relerr(ref_avg, ref_live))
    assert relerr(forward(), ref_live) < TOL      # the forward's slots are fresh again, for the live weights
    with L.opt.averaged_weights():
        assert all(stale for _, stale in L.slots_state()), "the exchange left a cached copy fresh"
        e = relerr(forward(), ref_avg)
        print("%s inside averaged_weights(): %.2e" % (name, e))
        assert e < TOL, (name, "inside", e)
    assert all(stale for _, stale in L.slots_state()), "the exchange back left a cached copy fresh"
    e = relerr(forward(), ref_live)
    print("%s after averaged_weights(): %.2e" % (name, e))
    assert e < TOL, (name, "after", e)
    if L.mods:
        u2, v2 = L.uv()[0]
        assert torch.equal(u2, uv[0]) and torch.equal(v2, uv[1]), "an eval-mode forward moved u / v"


# ------------------------------------------------------------------------------------------------------------------------------
# 6. the trainer
# ------------------------------------------------------------------------------------------------------------------------------
def _uv(*mods):
    return {"%d/%s" % (i, k): v.detach().clone() for i, mod in enumerate(mods) for k, v in mod.state_dict().items()
            if k.endswith(("weight_u", "weight_v"))}


def _oracle_state(mod, keys, params):
    """The module's buffers and the given parameter values as an fp64 oracle state dict, in load_keys order."""
    sd = mod.state_dict()
    return {k: (params[k] if k in params else _host(sd[k])).clone() for k, _ in keys}


def test_trainer_averaged_agents():
    import optimalstrategiesagainstgenerativeattacks_amd as G
    from optimalstrategiesagainstgenerativeattacks_amd import authentication_eval as ae
    from tests.test_gpu_models import _product_models
    tag, cfg = "wavg/tr", "16_1_32"
    B, m, n, k, c, s, d = 2, 1, 3, 4, 1, 16, 32
    lr = 1e-2
    keys = load_keys(cfg)
    with tempfile.TemporaryDirectory() as td:
        au, im = _product_models(tag, cfg)
        tr = G.GIMImgTrainer(os.path.join(td, "a"), m, n, k, au, im, lr, lr, lr, reg_param=0.0, im_ema_decay=DECAY, au_ema_decay=DECAY)
        assert tr.averages() and tr.impersonator_opt.averaging == DECAY and tr.authenticator_opt.averaging == DECAY
        trainer = G.DataParallelMock(tr)
        agents = {"im": (im, tr.impersonator_opt), "au": (au, tr.authenticator_opt)}
        named = {a: dict(mod.named_parameters()) for a, (mod, _) in agents.items()}
        recs = {a: _Recurrence(_read(named[a]), DECAY) for a in agents}      # the average starts as the weights at the build
        start = {a: _read(named[a]) for a in agents}
        for t, mbs in enumerate((1, 2)):
            ep = episode("%s/%d" % (tag, t), B, m, n, k, c, s, d)
            G.gim_step(trainer, *[x.float().to(dev()) for x in ep[:3]], z=ep[3].float().to(dev()), micro_batches=mbs)
            torch.cuda.synchronize()
            for a, (_, opt) in agents.items():
                recs[a].update(_read(named[a]))
                recs[a].check(_avg_by_name(opt, named[a]), "%s after gim_step %d (micro_batches %d)" % (a, t, mbs))
        for a, (_, opt) in agents.items():     # one update per step: with decay 0.5 a second one would be far outside the bound
            got = _avg_by_name(opt, named[a])
            moved = max(float((got[kk] - start[a][kk]).abs().max()) for kk in got)
            assert moved > 100 * recs[a].bound(), (a, moved)

        # ---- evaluation on the averaged weights
        leaked, real, si, z = episode(tag + "/eval", B, m, n, k, c, s, d)
        im_o = _oracle_state(im, keys["im"], _avg_by_name(tr.impersonator_opt, named["im"]))
        au_o = _oracle_state(au, keys["au"], _avg_by_name(tr.authenticator_opt, named["au"]))
        live = {a: {kk: p.detach().clone() for kk, p in named[a].items()} for a in agents}
        avg_dev = {a: {kk: opt.average_state()[p].detach().clone() for kk, p in named[a].items()} for a, (_, opt) in agents.items()}
        with torch.no_grad():
            fake_o = go.impersonator(im_o, leaked, n, z, False)
            out_o = go.authenticator(au_o, fake_o, si, False)
        au.train()
        im.train()
        uv_before = _uv(au, im)
        with tr.averaged():
            assert not any(mod.training for net in (au, im) for mod in net.modules()), "averaged() evaluates in eval mode"
            for a in agents:
                for kk, p in named[a].items():
                    assert torch.equal(p.detach(), avg_dev[a][kk]), (a, kk)
            fake = tr.forward(mode="impersonator_sample", leaked_sample=leaked.float().to(dev()), z=z.float().to(dev()))
            with torch.no_grad():
                out = au(test_sample=fake, si_sample=si.float().to(dev()))
            torch.cuda.synchronize()
        e_fake, e_out = relerr(fake, fake_o), relerr(out, out_o)
        print("averaged agents vs oracle on the averaged parameters: fake %.2e logits %.2e" % (e_fake, e_out))
        assert e_fake < 1e-3 and e_out < 1e-3, (e_fake, e_out)
        uv_after = _uv(au, im)
        for kk, v in uv_before.items():
            assert torch.equal(v, uv_after[kk]), (kk, "a spectral-norm vector moved inside averaged()")
        assert all(mod.training for net in (au, im) for mod in net.modules()), "the training flags were not restored"
        for a in agents:
            for kk, p in named[a].items():
                assert torch.equal(p.detach(), live[a][kk]), (a, kk, "the live weights did not come back")

        # ---- checkpoints
        tr.do_global_step()
        tr.save(epoch=0)
        path = os.path.join(tr.checkpoint_dir, "model_{:08}.pt".format(tr.global_step))
        payload = torch.load(path, map_location="cpu", weights_only=False)
        assert set(payload) == set(tr.CHECKPOINT_KEYS) | {"global_step", "last_epoch", "averaged"}
        assert set(payload["averaged"]) == {"impersonator", "authenticator"}
        assert payload["averaged"]["impersonator"]["decay"] == DECAY
        assert set(payload["averaged"]["impersonator"]["state"]) == set(named["im"])
        au2, im2 = _product_models(tag + "/other", cfg)
        tr2 = G.GIMImgTrainer(os.path.join(td, "b"), m, n, k, au2, im2, lr, lr, lr, reg_param=0.0, im_ema_decay=DECAY, au_ema_decay=DECAY)
        assert not torch.equal(dict(im2.named_parameters())["img2img.down_block.down_blocks.0.conv_r1.weight_orig"].detach(),
                               live["im"]["img2img.down_block.down_blocks.0.conv_r1.weight_orig"])
        tr2.resume_from_ckpt(path)
        agents2 = {"im": (im2, tr2.impersonator_opt), "au": (au2, tr2.authenticator_opt)}
        for a, (mod, opt) in agents2.items():
            avg2 = opt.average_state()
            for kk, p in mod.named_parameters():
                assert torch.equal(p.detach(), live[a][kk]), (a, kk, "resumed parameter")
                assert torch.equal(avg2[p], avg_dev[a][kk]), (a, kk, "resumed average")

        au3, im3 = _product_models(tag + "/plain", cfg)
        tr3 = G.GIMImgTrainer(os.path.join(td, "c"), m, n, k, au3, im3, lr, lr, lr, reg_param=0.0)
        assert not tr3.averages()
        tr3.do_global_step()
        tr3.save(epoch=0)
        path3 = os.path.join(tr3.checkpoint_dir, "model_{:08}.pt".format(tr3.global_step))
        assert set(torch.load(path3, map_location="cpu", weights_only=False)) == set(tr3.CHECKPOINT_KEYS) | {"global_step", "last_epoch"}
        tr2.resume_from_ckpt(path3)     # a file without the entry: the average starts from the loaded weights
        for a, (mod, opt) in agents2.items():
            avg2 = opt.average_state()
            src = dict((au3 if a == "au" else im3).named_parameters())
            for kk, p in mod.named_parameters():
                assert torch.equal(p.detach(), src[kk].detach()), (a, kk)
                assert torch.equal(avg2[p], p.detach()), (a, kk, "avg == p after a resume without the entry")

        # ---- authentication_eval
        args = {"img_size": s, "img_channels": c, "style_dim": d, "use_img_att": False, "num_env_noise_layers": 4, "remove_noise_mean": True}
        agent = ae.get_impersonator(dev(), "gim", path, None, args, averaged=True)
        for kk, p in agent.model.named_parameters():
            assert torch.equal(p.detach(), avg_dev["im"][kk]), (kk, "get_impersonator(averaged=True)")
        sd_live = agent.model.state_dict()
        for kk, v in uv_before.items():
            if kk.startswith("1/"):
                assert torch.equal(sd_live[kk[2:]], v), (kk, "the overlay keeps the live u / v")
        agent = ae.get_authenticator(dev(), "gim", path, args, averaged=True)
        for kk, p in agent.model.named_parameters():
            assert torch.equal(p.detach(), avg_dev["au"][kk]), (kk, "get_authenticator(averaged=True)")
        agent = ae.get_impersonator(dev(), "gim", path, None, args)
        for kk, p in agent.model.named_parameters():
            assert torch.equal(p.detach(), live["im"][kk]), (kk, "get_impersonator() keeps loading the live weights")
        for make in (lambda: ae.get_impersonator(dev(), "gim", path3, None, args, averaged=True),
                     lambda: ae.get_authenticator(dev(), "gim", path3, args, averaged=True)):
            with pytest.raises(KeyError, match="model_00000000.pt"):
                make()
