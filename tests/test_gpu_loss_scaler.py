"""GPU suite of the dynamic loss scale of the fp16 matrix path (GIM_FP16_LOSS_SCALE=dynamic / ops.set_loss_scale("dynamic")):

  1. gim_adam_step_scaled against gim_adam_step: the same update on a clean bucket, nothing touched on a poisoned one;
  2. the scaler's schedule (growth, backoff, floor) against a model written here;
  3. the non-saturating instantiations of the fp16 convolution kernels (gim_conv_shape.prec = 2), per kernel family, through
     ops.conv2d: bit-equal to the saturating ones in range, an infinity where those clip;
  4. a training step that overflows skips both updates, leaves nothing poisoned and recovers;
  5. the checkpoint entry "loss_scalers".

Every comparison here is exact (torch.equal, integers, finiteness): the scale is a power of two, so scaling and un-scaling do not
round, and the two conversions differ only beyond the fp16 range."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import portable_fill as pf
from tests.helpers import T, episode, epi_plan, filled_sd, load_keys

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture()
def fp16_det():
    """fp16 matrix path in deterministic mode; the loss-scale setting is restored afterwards."""
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    prev_path, prev_det, prev_scale = ops.set_matrix_path("fp16"), ops.set_deterministic(True), ops.set_loss_scale(4096)
    yield ops
    ops.set_loss_scale(prev_scale)
    ops.set_deterministic(prev_det)
    ops.set_matrix_path(prev_path)


# ---------------------------------------------------------------------------------------------------------------------
# 1. guarded Adam
# ---------------------------------------------------------------------------------------------------------------------
BETAS, EPS, GS = (0.5, 0.99), 1e-8, 0.5    # GS: the 1 / world_size factor of a two-rank job


def _words(scale=4096.0, interval=2000, clean=0, skipped=0, min_scale=1.0):
    from optimalstrategiesagainstgenerativeattacks_amd.optim import LossScaler
    sc = LossScaler(dev(), init=scale, growth_interval=interval, min_scale=min_scale)
    sc.load_state_dict({"clean_steps": clean, "skipped": skipped})
    return sc


def _bucket(n):
    """p, g, m, v of n floats in three segments (the middle one ends in 7 padding slots where n allows) and their learning rates."""
    gen = torch.Generator().manual_seed(n)
    p, g = torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 4096.0 * 1e-3
    m, v = torch.randn(n, generator=gen) * 1e-3, torch.rand(n, generator=gen) * 1e-6
    ends = sorted({max(1, n // 3), max(1, (2 * n) // 3), n})
    while len(ends) < 3:
        ends.append(n)        # (n = 1: empty trailing segments)
    pad = (ends[1] - min(7, ends[1] - ends[0]), ends[1])
    for t in (p, g, m, v):
        t[pad[0]:pad[1]] = 0.0
    seg = torch.tensor(ends, dtype=torch.int64, device=dev())
    lr = torch.tensor([1e-3, 3e-4, 1e-2], dtype=torch.float32, device=dev())
    return [t.to(dev()) for t in (p, g, m, v)], seg, lr, pad


def _adam(lib, name, bufs, seg, lr, grad_scale, step, state=None):
    from optimalstrategiesagainstgenerativeattacks_amd._lib import check
    p, g, m, v = bufs
    args = [p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), seg.data_ptr(), lr.data_ptr(), 3, BETAS[0], BETAS[1], EPS,
            grad_scale, step.data_ptr()]
    if state is not None:
        args.append(state.words.data_ptr())
    check(getattr(lib, name)(*args, torch.cuda.current_stream().cuda_stream), name)


ADAM_SIZES = [1, 255, 1025, 4096 * 1024 + 5]     # the last one: more than 4096 blocks of 1024 elements - the block cap is active


@pytest.mark.parametrize("n", ADAM_SIZES)
def test_guarded_adam_matches_adam_on_a_clean_bucket_and_skips_a_poisoned_one(n):
    from optimalstrategiesagainstgenerativeattacks_amd import _lib
    lib = _lib.load()
    bufs, seg, lr, pad = _bucket(n)
    # clean: the update of gim_adam_step with grad_scale / 4096
    ref = [t.clone() for t in bufs]
    step_ref = torch.full((1,), 4, dtype=torch.int32, device=dev())
    _adam(lib, "gim_adam_step", ref, seg, lr, GS / 4096.0, step_ref)
    got = [t.clone() for t in bufs]
    step, sc = torch.full((1,), 4, dtype=torch.int32, device=dev()), _words(clean=5)
    _adam(lib, "gim_adam_step_scaled", got, seg, lr, GS, step, sc)
    for name, a, b in zip("pmv", (got[0], got[2], got[3]), (ref[0], ref[2], ref[3])):
        assert torch.equal(a, b), name
    assert not torch.equal(got[0], bufs[0]), "the update did not run"
    st = sc.state()
    assert int(step) == int(step_ref) == 5 and st["clean_steps"] == 6 and st["skipped"] == 0 and st["scale"] == 4096.0
    assert not st["last_overflow"] and int(sc.words[4]) == 0
    # poisoned: nothing moves, the scale halves
    poisons = [(0, float("inf")), (n - 1, float("-inf")), (n // 2, float("nan"))]
    if pad[1] > pad[0]:
        poisons.append((pad[0], float("nan")))            # a padding slot between two segments
    for idx, val in poisons:
        cur = [t.clone() for t in bufs]
        cur[1][idx] = val
        step, sc = torch.full((1,), 4, dtype=torch.int32, device=dev()), _words(clean=5, skipped=2)
        _adam(lib, "gim_adam_step_scaled", cur, seg, lr, GS, step, sc)
        for name, a, b in zip("pmv", (cur[0], cur[2], cur[3]), (bufs[0], bufs[2], bufs[3])):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (name, idx, val)
        st = sc.state()
        assert int(step) == 4 and st["scale"] == 2048.0 and st["skipped"] == 3 and st["clean_steps"] == 0, (idx, val, st)
        assert st["last_overflow"] and int(sc.words[4]) == 0, (idx, val)
        assert float(sc.words[1:2].view(torch.float32)) == 1.0 / 2048.0


# ---------------------------------------------------------------------------------------------------------------------
# 2. schedule
# ---------------------------------------------------------------------------------------------------------------------
def test_scaler_schedule_follows_the_model():
    from optimalstrategiesagainstgenerativeattacks_amd import _lib
    lib = _lib.load()
    bufs, seg, lr, _ = _bucket(64)
    interval, floor = 3, 1024.0
    sc, step = _words(scale=4096.0, interval=interval, min_scale=floor), torch.zeros(1, dtype=torch.int32, device=dev())
    # c = clean, x = poisoned: growth after exactly three clean steps (twice), a count reset by an overflow, two overflows in a
    # row (2048, 1024), and the floor (2048 -> 1024 -> 1024 -> 1024)
    script = "ccccxccxxcccxxxc"
    scale, clean, skipped, t = 4096.0, 0, 0, 0
    seen = set()
    for i, ev in enumerate(script):
        bufs[1].normal_()
        if ev == "x":
            bufs[1][(7 * i) % 64] = float("inf") if i % 2 else float("nan")
        _adam(lib, "gim_adam_step_scaled", bufs, seg, lr, 1.0, step, sc)
        # the model
        if ev == "x":
            at_floor = scale * 0.5 < floor
            scale, clean, skipped = max(scale * 0.5, floor), 0, skipped + 1
            seen.add("floor" if at_floor else "backoff")
        else:
            t, clean = t + 1, clean + 1
            if clean == interval:
                scale, clean = scale * 2.0, 0
                seen.add("growth")
        st = sc.state()
        assert (st["scale"], st["clean_steps"], st["skipped"], int(step)) == (scale, clean, skipped, t), (i, ev, st, int(step))
        assert st["last_overflow"] == (ev == "x")
    assert seen == {"floor", "backoff", "growth"} and scale == 1024.0
    assert all(torch.isfinite(b).all() for b in (bufs[0], bufs[2], bufs[3]))


# ---------------------------------------------------------------------------------------------------------------------
# 3. non-saturating kernels per family
# ---------------------------------------------------------------------------------------------------------------------
CONV_CASES = {
    # name: (N, S, Cin, Cout, K, pool)
    "3x3_patch_fastb": (2, 8, 32, 64, 3, False),     # patch-resident forward and dgrad_t; FASTB weight gradient
    "1x1": (4, 16, 64, 128, 1, False),
    "2x2_maps_splitk": (70, 2, 128, 128, 3, False),  # split-K forward-style launches, generic gather in the weight gradient
    "pool_folded": (3, 16, 64, 64, 3, True),         # stride-2 gather
}
_CONV_INPUTS = {}


def _conv_inputs(name):
    """x, w, b and an in-range dy of a case on the device, made once."""
    if name not in _CONV_INPUTS:
        N, S, Cin, Cout, K, pool = CONV_CASES[name]
        So = S // 2 if pool else S
        x = T(pf.normal(name + "/lsx", (N, S, S, Cin)), torch.float32).to(dev())
        w = T(pf.normal(name + "/lsw", (Cout, Cin, K, K)) / np.sqrt(Cin * K * K), torch.float32).to(dev()).contiguous(memory_format=torch.channels_last)
        b = T(pf.normal(name + "/lsb", (Cout,)), torch.float32).to(dev())
        dy = T(pf.uniform(name + "/lsdy", (N, So, So, Cout)), torch.float32).to(dev())
        _CONV_INPUTS[name] = (x, w, b, dy)
    return _CONV_INPUTS[name]


def _conv_grads(ops, name, dy, scaler):
    """dx, dw, db of ops.conv2d on the fp16 path; the backward pass armed by `scaler` (None: un-armed, prec = 1)."""
    N, S, Cin, Cout, K, pool = CONV_CASES[name]
    x, w, b, _ = _conv_inputs(name)
    x, w, b = x.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
    y = ops.conv2d(x, w, b, None, None, None, None, 0, 0.2, pool)
    with ops.armed_backward(scaler):
        (y * dy).sum().backward()
    return x.grad, w.grad, b.grad


@pytest.mark.parametrize("name", list(CONV_CASES))
def test_non_saturating_kernels_per_family(name, fp16_det):
    ops = fp16_det
    from optimalstrategiesagainstgenerativeattacks_amd.optim import LossScaler
    N, S, Cin, Cout, K, pool = CONV_CASES[name]
    sh = ops._shape(N, S, S, Cin, Cout, K, 0, 0.2, 1 if pool else 0, 1 if pool else 0)
    for kind in (0, 2, 3):
        assert epi_plan(sh, kind)[7] & 255 == 2, ("launch kind %d is not on the fp16 path" % kind, epi_plan(sh, kind))
    scaler = LossScaler(dev())
    _, _, _, dy = _conv_inputs(name)
    # (a) in range: the two instantiations agree to the bit
    sat, ieee = _conv_grads(ops, name, dy, None), _conv_grads(ops, name, dy, scaler)
    for what, a, b in zip(("dx", "dw", "db"), sat, ieee):
        assert torch.isfinite(a).all() and torch.equal(a, b), what
    for where in ((0, 0, 0, 0), (-1, -1, -1, -1)):
        # (b) one element beyond the fp16 range: clipped un-armed, an infinity armed
        big = dy.clone()
        big[where] = 7.0e4
        sat, ieee = _conv_grads(ops, name, big, None), _conv_grads(ops, name, big, scaler)
        assert all(torch.isfinite(t).all() for t in sat), "un-armed: today's clipping keeps everything finite"
        assert not torch.isfinite(ieee[0]).all(), ("dx", where)
        assert not torch.isfinite(ieee[1]).all(), ("dw", where)
        # (c) the largest finite fp16 value: nothing to clip, nothing overflows
        edge = dy.clone()
        edge[where] = 65504.0
        sat, ieee = _conv_grads(ops, name, edge, None), _conv_grads(ops, name, edge, scaler)
        for what, a, b in zip(("dx", "dw", "db"), sat, ieee):
            assert torch.isfinite(a).all() and torch.equal(a, b), (what, where)


# ---------------------------------------------------------------------------------------------------------------------
# 4. / 5. training steps and checkpoints.  Config 16_1_32 (the smallest golden one): its 32-channel 3x3 convolutions on 16x16 and
# 8x8 maps are fp16-eligible, which _assert_fp16_launches checks on the shapes the armed backward really built.
# ---------------------------------------------------------------------------------------------------------------------
CFG, DIMS = "16_1_32", dict(B=2, m=1, n=3, k=4, c=1, s=16, d=32)


def _trainer(tag, outdir):
    import optimalstrategiesagainstgenerativeattacks_amd as G
    keys = load_keys(CFG)
    au, im = G.get_au(DIMS["s"], DIMS["c"], DIMS["d"]), G.get_im(DIMS["s"], DIMS["c"], DIMS["d"])
    au.load_state_dict(filled_sd(keys["au"], tag + "/au/", torch.float32))
    im.load_state_dict(filled_sd(keys["im"], tag + "/im/", torch.float32))
    tr = G.GIMImgTrainer(str(outdir), DIMS["m"], DIMS["n"], DIMS["k"], au.to(dev()), im.to(dev()), 1e-3, 1e-3, 1e-4, reg_param=0.0)
    return tr


def _episode(tag, it):
    d = DIMS
    return [t.float().to(dev()) for t in episode("%s/%d" % (tag, it), d["B"], d["m"], d["n"], d["k"], d["c"], d["s"], d["d"])]


def _iterate(tr, tag, its):
    import optimalstrategiesagainstgenerativeattacks_amd as G
    outs = []
    for it in its:
        leaked, real, si, z = _episode(tag, it)
        gi, di = G.gim_step(G.DataParallelMock(tr), leaked, real, si, z=z)
        outs += list(gi) + list(di)
    torch.cuda.synchronize()
    return outs


def _snapshot(tr):
    """Every parameter and buffer (u / v of the spectral norms included) and both optimizers' moments."""
    snap = {"au/" + k: v.detach().clone() for k, v in tr.authenticator.state_dict().items()}
    snap.update({"im/" + k: v.detach().clone() for k, v in tr.impersonator.state_dict().items()})
    for name, opt in (("au_opt", tr.authenticator_opt), ("im_opt", tr.impersonator_opt)):
        snap[name + "/m"], snap[name + "/v"] = opt.flat_m.clone(), opt.flat_v.clone()
    return snap


def _params(snap):
    return {k: v for k, v in snap.items() if not k.endswith(("weight_u", "weight_v"))}


def _assert_fp16_launches(ops):
    from optimalstrategiesagainstgenerativeattacks_amd import _lib
    armed = [k for k in ops._SHAPES if k[-1] == 2]
    forms = set()
    for key in armed:
        sh = ops._SHAPES[key]
        for kind in (0, 2, 3):
            out = (ctypes.c_int32 * 8)()     # (a shape is planned for every kind here; one that a kind refuses just does not count)
            if _lib.load().gim_conv_launch_plan(ctypes.byref(sh), kind, ctypes.cast(out, ctypes.c_void_p)) == 0 and out[7] & 255 == 2:
                forms.add(kind)
    assert forms, "no armed launch of this config is fp16-eligible (%d armed shapes): take the next config" % len(armed)


def test_dynamic_mode_equals_static_mode_while_nothing_overflows(fp16_det, tmp_path):
    ops = fp16_det
    tag = "lsdyn"
    ops.set_loss_scale(4096)
    tr_s = _trainer(tag, tmp_path / "s")
    outs_s = _iterate(tr_s, tag, range(3))
    assert tr_s.authenticator_opt.loss_scaler is None and tr_s.impersonator_opt.loss_scaler is None
    ops.set_loss_scale("dynamic", init=4096)
    ops._SHAPES.clear()
    tr_d = _trainer(tag, tmp_path / "d")
    outs_d = _iterate(tr_d, tag, range(3))
    _assert_fp16_launches(ops)
    snap_s, snap_d = _snapshot(tr_s), _snapshot(tr_d)
    diff = [k for k in snap_s if not torch.equal(snap_s[k], snap_d[k])]
    assert not diff, "tensors that differ between static and dynamic mode: %s" % diff[:8]
    assert len(outs_s) == len(outs_d) and all(torch.equal(a, b) for a, b in zip(outs_s, outs_d))
    for opt in (tr_d.authenticator_opt, tr_d.impersonator_opt):
        st = opt.loss_scaler.state()
        assert (st["scale"], st["clean_steps"], st["skipped"]) == (4096.0, 3, 0), st
        assert int(opt._step_dev) == 3


def _overflowed_trainer(ops, tag, outdir):
    """A dynamic-mode trainer after ONE iteration from scale 2^100: both updates skipped.  -> (trainer, snapshot before, outputs)."""
    ops.set_loss_scale("dynamic", init=2.0 ** 100)
    tr = _trainer(tag, outdir)
    tr.authenticator_opt._ensure()
    tr.impersonator_opt._ensure()
    before = _snapshot(tr)
    outs = _iterate(tr, tag, [0])
    return tr, before, outs


def test_an_overflowing_step_is_skipped_and_the_next_one_recovers(fp16_det, tmp_path):
    import optimalstrategiesagainstgenerativeattacks_amd as G
    ops = fp16_det
    tag = "lsskip"
    tr, before, outs = _overflowed_trainer(ops, tag, tmp_path)
    after = _snapshot(tr)
    diff = [k for k in _params(before) if not torch.equal(before[k], after[k])]     # (no NaN in either: equal values = equal bits)
    assert not diff, "a skipped step moved %s" % diff[:8]
    for opt in (tr.authenticator_opt, tr.impersonator_opt):
        st = opt.loss_scaler.state()
        assert int(opt._step_dev) == 0 and st["scale"] == 2.0 ** 99 and st["skipped"] == 1 and st["last_overflow"], st
    assert torch.isfinite(outs[0]).all() and torch.isfinite(outs[3]).all(), "the returned losses are those of the un-scaled forward"
    # back to a usable scale: the step runs, and nothing of the skipped one is left behind
    for opt in (tr.authenticator_opt, tr.impersonator_opt):
        opt.loss_scaler.load_state_dict(dict(opt.loss_scaler.state_dict(), scale=4096.0))
    _iterate(tr, tag, [1])
    moved = _snapshot(tr)
    for agent in ("au/", "im/"):
        ks = [k for k in _params(after) if k.startswith(agent) and after[k].dtype == torch.float32]
        assert any(not torch.equal(after[k], moved[k]) for k in ks), agent
    assert all(torch.isfinite(v).all() for v in moved.values() if v.dtype == torch.float32)
    for opt in (tr.authenticator_opt, tr.impersonator_opt):
        st = opt.loss_scaler.state()
        assert st["skipped"] == 1 and st["clean_steps"] == 1 and st["scale"] == 4096.0 and int(opt._step_dev) == 1, st
    leaked, real, si, z = _episode(tag, 2)
    trainer = G.DataParallelMock(tr)
    g_loss, fake, _ = G.im_eval_step(trainer, leaked, si, z=z)
    d_loss = G.au_eval_step(trainer, real, fake, si)[0]
    assert torch.isfinite(g_loss).all() and torch.isfinite(d_loss).all()


def test_checkpoint_carries_the_loss_scalers_in_dynamic_mode_only(fp16_det, tmp_path):
    ops = fp16_det
    tag = "lsckpt"
    tr, _, _ = _overflowed_trainer(ops, tag, tmp_path / "a")
    tr.save(epoch=0)
    path = os.path.join(tr.checkpoint_dir, "model_%08d.pt" % tr.global_step)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert set(ck["loss_scalers"]) == {"authenticator_opt", "impersonator_opt"}
    assert all(int(s["step"]) == 0 for s in ck["impersonator_opt"]["state"].values()), "a skipped step must not count"
    fresh = _trainer(tag + "/other", tmp_path / "b")
    fresh.resume_from_ckpt(path)
    for opt in (fresh.authenticator_opt, fresh.impersonator_opt):
        st = opt.loss_scaler.state()
        assert (st["scale"], st["clean_steps"], st["skipped"]) == (2.0 ** 99, 0, 1), st
        assert all(int(s["step"]) == 0 for s in opt.state_dict()["state"].values())
    # a checkpoint the reference wrote has no such entry: it loads, and the scalers are the defaults
    import optimalstrategiesagainstgenerativeattacks_amd as G
    from tests.helpers import load_json
    c = load_json("ref_ckpt.json")["config"]
    ops.set_loss_scale("dynamic")
    au, im = G.get_au(c["s"], c["c"], c["d"]).to(dev()), G.get_im(c["s"], c["c"], c["d"]).to(dev())
    ref_tr = G.GIMImgTrainer(str(tmp_path / "c"), c["m"], c["n"], c["k"], au, im, au_lr=c["au_lr"], im_lr=c["im_lr"],
                             env_noise_mapping_lr=c["noise_lr"], reg_param=0.0)
    ref_tr.resume_from_ckpt(os.path.join(GOLDEN, "ref_ckpt_model_00000002.pt"))
    assert ref_tr.global_step == 2
    for opt in (ref_tr.authenticator_opt, ref_tr.impersonator_opt):
        st = opt.dynamic_scaler().state()
        assert (st["scale"], st["clean_steps"], st["skipped"], st["growth_interval"], st["min_scale"]) == (4096.0, 0, 0, 2000, 1.0), st
    # static mode: the reference's keys only
    ops.set_loss_scale(4096)
    ref_tr.save(epoch=0)
    ck = torch.load(os.path.join(ref_tr.checkpoint_dir, "model_%08d.pt" % ref_tr.global_step), map_location="cpu", weights_only=False)
    assert "loss_scalers" not in ck
    assert set(ck) == set(torch.load(os.path.join(GOLDEN, "ref_ckpt_model_00000002.pt"), map_location="cpu", weights_only=False))
