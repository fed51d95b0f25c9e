"""Gradient accumulation on the GPU: one GIM step over micro_batches = A equal slices of the batch is the step on the whole batch -
forward values, spectral-norm state, one Adam update with the mean gradient, one loss-scale decision.  Tiny configuration of the
data-parallel test (nets 16_1_32, m 1, n 3, k 4, 16x16x1, style 32), B = 4, explicit z, deterministic mode unless noted.

Bounds.  "bits": torch.equal.  "mean": 1e-6 relative - a mean of A slice means against the mean over the batch, in fp32.  "order": the
project's bounds for the same gradients added in another order (test_two_rank_data_parallel_step_on_gpu): worst tensor error 2e-3
for weights, 6e-2 for biases (a bias in front of a norm layer has a zero gradient, which Adam with beta1 = 0 turns into +-lr steps).
"oracle": _assert_one_adam_step_matches_oracle with max_share = max(3 x floor, 1e-3), the floor measured here on the fp32 oracle."""
import gc
import os
import subprocess
import sys
import tempfile

import pytest
import torch

from oracle import gim_oracle as go
from tests.helpers import episode, filled_sd, load_keys, relerr
from tests.test_gpu_models import _adam_step_off_shares, _assert_one_adam_step_matches_oracle

pytestmark = pytest.mark.gpu

CFG = "16_1_32"
M, N, K, C, S, D = 1, 3, 4, 1, 16, 32
LRS = {"au": 1e-3, "im": 1e-3}
TAG = "acc"
W_BOUND, B_BOUND = 2e-3, 6e-2


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture()
def det():
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    prev = ops.set_deterministic(True)
    yield ops
    ops.set_deterministic(prev)


def _trainer(tag=TAG, reg_param=0.0, outdir=None):
    import optimalstrategiesagainstgenerativeattacks_amd as G
    keys = load_keys(CFG)
    au, im = G.get_au(S, C, D), G.get_im(S, C, D)
    au.load_state_dict(filled_sd(keys["au"], tag + "/au/", torch.float32))
    im.load_state_dict(filled_sd(keys["im"], tag + "/im/", torch.float32))
    with tempfile.TemporaryDirectory() as td:
        tr = G.GIMImgTrainer(outdir or td, M, N, K, au.to(dev()), im.to(dev()), LRS["au"], LRS["im"], 1e-4, reg_param=reg_param)
    tr.authenticator_opt._ensure()
    tr.impersonator_opt._ensure()
    return tr


def _batch(it, B=4, tag=TAG):
    return [t.float().to(dev()) for t in episode("%s/%d" % (tag, it), B, M, N, K, C, S, D)]


def _snapshot(tr):
    """Parameters, spectral-norm buffers, Adam moments and step counters."""
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    ops.join_lanes()
    torch.cuda.synchronize()
    snap = {"au." + k: v.detach().clone() for k, v in tr.authenticator.state_dict().items()}
    snap.update({"im." + k: v.detach().clone() for k, v in tr.impersonator.state_dict().items()})
    for name, opt in (("au_opt", tr.authenticator_opt), ("im_opt", tr.impersonator_opt)):
        snap[name + "/m"], snap[name + "/v"], snap[name + "/step"] = opt.flat_m.clone(), opt.flat_v.clone(), opt._step_dev.clone()
    return snap


def _is_sn(k):
    return k.endswith(("weight_u", "weight_v"))


def _run(iters, A, reg_param=0.0, B=4, tag=TAG, pass_kw=True):
    """`iters` iterations of gim_step from the filled weights -> (trainer, [(gi, di)], snapshot)."""
    import optimalstrategiesagainstgenerativeattacks_amd as G
    tr = _trainer(tag, reg_param)
    trainer = G.DataParallelMock(tr)
    kw = {"micro_batches": A} if pass_kw else {}
    outs = []
    for it in range(iters):
        leaked, real, si, z = _batch(it, B, tag)
        tr.do_global_step()
        outs.append(G.gim_step(trainer, leaked, real, si, z=z, **kw))
    snap = _snapshot(tr)
    return tr, outs, snap


_RUNS = {}


def _shared_run(iters, A, reg_param=0.0):
    """Runs that several tests read (deterministic mode, fp32): made once, left unchanged."""
    key = (iters, A, reg_param)
    if key not in _RUNS:
        _, outs, snap = _run(iters, A, reg_param, pass_kw=A > 1)
        _RUNS[key] = ([tuple(tuple(t.clone() for t in part) for part in o) for o in outs], snap)
    return _RUNS[key]


def _worst(snap_a, snap_b):
    ww = wb = 0.0
    for k in snap_b:
        if "_opt/" in k:
            continue
        e = relerr(snap_a[k], snap_b[k])
        if k.endswith(".bias"):
            wb = max(wb, e)
        else:
            ww = max(ww, e)
    return ww, wb


def _assert_order_bounds(what, snap_a, snap_b):
    ww, wb = _worst(snap_a, snap_b)
    print("%s, worst tensor error: weights %.2e (bound %.0e), biases %.2e (bound %.0e)" % (what, ww, W_BOUND, wb, B_BOUND))
    assert ww < W_BOUND and wb < B_BOUND, (what, ww, wb)


def _close_mean(a, b, scale=None):
    a, b = float(a), float(b)
    return abs(a - b) <= 1e-6 * max(abs(b), scale or 0.0)


# 1 ---------------------------------------------------------------------------------------------------------------------
def test_accumulated_forward_is_the_whole_batch_forward(det):
    """Per-episode logits, fake samples and predictions of one gim_step(micro_batches=2) are bit-identical to the plain step's
    from the same weights; the mean losses agree to the rounding of an fp32 mean (1e-6 relative; the two mean logits, which
    cancel, relative to 1 - the size of a logit)."""
    (gi_w, di_w), = _shared_run(1, 1)[0]
    (gi_a, di_a), = _shared_run(1, 2)[0]
    assert gi_a[1].shape == gi_w[1].shape == (4, N, C, S, S) and gi_a[2].shape == gi_w[2].shape
    assert torch.equal(gi_a[2], gi_w[2]), "logits on the fake sets, per episode"
    assert torch.equal(gi_a[1], gi_w[1]), "fake_sample"
    assert torch.equal(di_a[8], di_w[8]) and torch.equal(di_a[8], gi_w[1])
    assert di_a[6].shape == di_w[6].shape and torch.equal(di_a[6], di_w[6]) and torch.equal(di_a[7], di_w[7]), "predictions"
    for i, what in ((0, "generator loss"),):
        print("%s: accumulated %.9g whole batch %.9g" % (what, float(gi_a[i]), float(gi_w[i])))
        assert gi_a[i].shape == gi_w[i].shape and _close_mean(gi_a[i], gi_w[i]), what
    for i, what in ((0, "discriminator loss"), (1, "loss on real"), (2, "loss on fake"), (3, "R1 term"), (4, "mean logit on real"),
                    (5, "mean logit on fake")):
        print("%s: accumulated %.9g whole batch %.9g" % (what, float(di_a[i]), float(di_w[i])))
        assert di_a[i].shape == di_w[i].shape and _close_mean(di_a[i], di_w[i], 1.0 if i >= 4 else None), what


# 2 ---------------------------------------------------------------------------------------------------------------------
def test_accumulated_step_advances_spectral_norm_once(det):
    """Every weight_u / weight_v of both networks after the accumulated step is bit-identical to the whole-batch step's.  Control: a
    hand-written loop of plain forwards on the two halves - what a caller without the feature would write - leaves other u."""
    import optimalstrategiesagainstgenerativeattacks_amd as G
    snap_w, snap_a = _shared_run(1, 1)[1], _shared_run(1, 2)[1]
    sn_keys = [k for k in snap_w if _is_sn(k)]
    assert len(sn_keys) > 100
    diff = [k for k in sn_keys if not torch.equal(snap_w[k], snap_a[k])]
    assert not diff, "spectral-norm buffers that differ from the whole-batch step's: %s" % diff[:8]
    # control
    tr = _trainer()
    trainer = G.DataParallelMock(tr)
    leaked, real, si, z = _batch(0)
    tr.impersonator.train()
    tr.authenticator.train()
    with torch.no_grad():
        for h in range(2):
            sl = slice(2 * h, 2 * h + 2)
            _, fake, _ = trainer.forward(mode='impersonator_forward', leaked_sample=leaked[sl], si_sample=si[sl], z=z[sl])
            trainer.forward(mode='authenticator_forward', fake_sample=fake, real_sample=real[sl], si_sample=si[sl], grad=False)
    snap_c = _snapshot(tr)
    for agent in ("au.", "im.src_encoder", "im.img2img"):
        ks = [k for k in sn_keys if k.startswith(agent) and k.endswith("weight_u")]
        moved = [k for k in ks if not torch.equal(snap_c[k], snap_w[k])]
        print("control, %s: %d of %d weight_u differ from the whole-batch step's" % (agent, len(moved), len(ks)))
        assert ks and moved, (agent, len(moved), len(ks))


# 3 ---------------------------------------------------------------------------------------------------------------------
_ORACLE = {}


def _oracle_step():
    """The fp64 oracle's step on all four episodes and the fp32 oracle's floor, as test_two_rank_data_parallel_step_on_gpu makes them."""
    if not _ORACLE:
        keys = load_keys(CFG)
        leaked, real, si, z = episode(TAG + "/0", 4, M, N, K, C, S, D)
        otr = go.OracleTrainer(filled_sd(keys["au"], TAG + "/au/"), filled_sd(keys["im"], TAG + "/im/"), N, LRS["au"], LRS["im"], 1e-4)
        g_o, d_o = otr.step(leaked, real, si, z)
        otr32 = go.OracleTrainer({k_: v.float() for k_, v in filled_sd(keys["au"], TAG + "/au/").items()},
                                 {k_: v.float() for k_, v in filled_sd(keys["im"], TAG + "/im/").items()}, N, LRS["au"], LRS["im"], 1e-4)
        otr32.step(*[t.float() for t in (leaked, real, si, z)])
        p32 = {nm: {k_: v for k_, v in sd_.items() if go.is_param(k_)} for nm, sd_ in (("au", otr32.au_sd), ("im", otr32.im_sd))}
        floor = max(v[0] for v in _adam_step_off_shares(p32, otr, LRS).values())
        print("fp32 oracle vs fp64 oracle: worst share of elements off by > 0.05 lr after one Adam step: %.2e" % floor)
        _ORACLE.update(otr=otr, g_o=g_o, d_o=d_o, floor=floor)
    return _ORACLE


@pytest.mark.parametrize("A", [2, 4])
def test_accumulated_step_vs_oracle_on_the_whole_batch(det, A):
    o = _oracle_step()
    outs, snap = _shared_run(1, A)
    (gi, di), = outs
    g_o, d_o = o["g_o"], o["d_o"]
    errs = (relerr(gi[0], g_o[0].mean()), relerr(di[0], d_o[0].mean()), abs(float(di[4]) - float(d_o[4].mean())))
    print("A = %d: generator loss %.2e, discriminator loss %.2e (relative), mean logit on real %.2e (absolute)" % ((A,) + errs))
    assert errs[0] < 1e-3 and errs[1] < 1e-3
    assert errs[2] < 1e-3 * abs(float(d_o[4].mean())) + 1e-5
    params = {nm: {k_[3:]: v for k_, v in snap.items() if k_.startswith(nm + ".") and not _is_sn(k_)} for nm in ("au", "im")}
    bufs = {nm: {k_[3:]: v for k_, v in snap.items() if k_.startswith(nm + ".") and _is_sn(k_)} for nm in ("au", "im")}
    shares = _adam_step_off_shares(params, o["otr"], LRS)
    print("A = %d: worst share of elements off the oracle's update by > 0.05 lr: %.2e (bound %.2e)"
          % (A, max(v[0] for v in shares.values()), max(3 * o["floor"], 1e-3)))
    _assert_one_adam_step_matches_oracle(params, bufs, o["otr"], LRS, max_share=max(3 * o["floor"], 1e-3))
    assert int(snap["au_opt/step"]) == 1 and int(snap["im_opt/step"]) == 1, "one Adam update per optimizer"


# 4 ---------------------------------------------------------------------------------------------------------------------
def test_two_accumulated_iterations_vs_two_plain_iterations(det):
    snap_w, snap_a = _shared_run(2, 1)[1], _shared_run(2, 2)[1]
    _assert_order_bounds("2 micro-batches vs whole batch after two iterations", snap_a, snap_w)
    for name in ("au_opt", "im_opt"):
        assert int(snap_a[name + "/step"]) == int(snap_w[name + "/step"]) == 2
    diff = [k for k in snap_w if _is_sn(k) and relerr(snap_a[k], snap_w[k]) > W_BOUND]
    assert not diff, diff[:8]


# 5 ---------------------------------------------------------------------------------------------------------------------
def test_accumulated_r1_step(det):
    """reg_param = 10: the second-order launches run once per micro-batch; one iteration, the "order" bounds."""
    (_, di_w), = _shared_run(1, 1, 10.0)[0]
    (_, di_a), = _shared_run(1, 2, 10.0)[0]
    print("R1 term: accumulated %.9g whole batch %.9g" % (float(di_a[3]), float(di_w[3])))
    assert float(di_w[3]) > 0 and relerr(di_a[3], di_w[3]) < 1e-3
    _assert_order_bounds("R1, 2 micro-batches vs whole batch after one iteration", _shared_run(1, 2, 10.0)[1], _shared_run(1, 1, 10.0)[1])


# 6 ---------------------------------------------------------------------------------------------------------------------
def test_one_micro_batch_is_the_plain_path(det):
    _, outs_n, snap_n = _run(3, 1, pass_kw=False)
    _, outs_1, snap_1 = _run(3, 1, pass_kw=True)
    diff = [k for k in snap_n if not torch.equal(snap_n[k], snap_1[k])]
    assert not diff, "micro_batches=1 differs from the plain call in %s" % diff[:8]
    for (gn, dn), (g1, d1) in zip(outs_n, outs_1):
        assert all(torch.equal(a, b) for a, b in zip(gn + dn, g1 + d1))
    assert int(snap_1["au_opt/step"]) == 3


# 7 ---------------------------------------------------------------------------------------------------------------------
def test_accumulated_step_is_bit_reproducible(det):
    outs_a, snap_a = _shared_run(1, 2)
    _, outs_b, snap_b = _run(1, 2)
    diff = [k for k in snap_a if not torch.equal(snap_a[k], snap_b[k])]
    assert not diff, "tensors that differ between two deterministic accumulated runs: %s" % diff[:8]
    assert all(torch.equal(a, b) for a, b in zip(outs_a[0][0] + outs_a[0][1], outs_b[0][0] + outs_b[0][1]))


# 8 ---------------------------------------------------------------------------------------------------------------------
def test_train_epoch_with_two_discriminator_steps_per_generator_step(det, tmp_path):
    """n_au_steps = 2 through train_epoch on a synthetic bank: the iterations in which the generator only evaluates (while the
    authenticator stays in train mode and advances its u) accumulate too.  Same seeded batches and z with micro_batches 2 and 1."""
    import optimalstrategiesagainstgenerativeattacks_amd as G
    from optimalstrategiesagainstgenerativeattacks_amd import gim_img_training as gt
    from optimalstrategiesagainstgenerativeattacks_amd.training_logger import Logger

    def run(A):
        out = tmp_path / ("a%d" % A)
        tr = _trainer("acc8", outdir=str(out))
        imgs, offs = G.synthetic_bank(6, 10, S, C, dev(), seed=1)
        tr_ds = G.EpisodeBank(imgs, offs, M, N, K, example_cnt_per_class=2, mirror=True, seed=21)
        va_ds = G.EpisodeBank(imgs, offs, M, N, K, example_cnt_per_class=1, mirror=False, seed=22)
        logger = Logger(log_dir=str(out / "logs"), img_dir=str(out / "imgs"), tensorboard_dir=str(out / "tb"))
        torch.manual_seed(77)
        gt.train_epoch(device=dev(), logger=logger, epoch=0, trainer=G.DataParallelMock(tr), train_ds=tr_ds, val_ds=va_ds,
                       train_batch_size=4, val_batch_size=4, num_workers=0, save_every=1000, eval_every=2, save_imgs_every=1000,
                       train_eval_indices=[0], val_eval_indices=[1], tb_log_every=1, tb_log_enc_every=1000, n_au_steps=2,
                       **({"micro_batches": A} if A > 1 else {}))
        assert tr.global_step == 2
        return logger.stats, _snapshot(tr)
    st_w, snap_w = run(1)
    st_a, snap_a = run(2)
    cats = ("train_losses", "train_au_out", "train_accuracy", "train losses", "lr")
    for cat in cats:
        assert set(st_a[cat]) == set(st_w[cat]), cat
        for k in st_w[cat]:
            assert [s_ for s_, _ in st_a[cat][k]] == [s_ for s_, _ in st_w[cat][k]] == [0, 1, 2], (cat, k)
    for cat, k in (("train_losses", "dis_loss"), ("train_losses", "dis_loss_on_real"), ("train_losses", "dis_loss_on_fake"),
                   ("train losses", "gen loss")):
        a, w = st_a[cat][k][0][1], st_w[cat][k][0][1]
        print("iteration 0 %s / %s: accumulated %.9g whole batch %.9g" % (cat, k, a, w))
        assert abs(a - w) < 1e-3 * abs(w), (cat, k)
    assert int(snap_a["au_opt/step"]) == int(snap_w["au_opt/step"]) == 3 and int(snap_a["im_opt/step"]) == int(snap_w["im_opt/step"]) == 1
    _assert_order_bounds("train_epoch, n_au_steps 2, three iterations", snap_a, snap_w)


# 9 ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def fp16_det():
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    prev_path, prev_det, prev_scale = ops.set_matrix_path("fp16"), ops.set_deterministic(True), ops.set_loss_scale(4096)
    yield ops
    ops.set_loss_scale(prev_scale)
    ops.set_deterministic(prev_det)
    ops.set_matrix_path(prev_path)


def test_fp16_overflow_in_an_accumulated_step_skips_one_update(fp16_det):
    """Dynamic scale 2^100 (the means of tests/test_gpu_loss_scaler.py): the backward passes overflow - arithmetic, no fault - and the
    infinity in the bucket makes the guarded Adam skip the ONE update of each optimizer and halve its scale once."""
    import optimalstrategiesagainstgenerativeattacks_amd as G
    ops = fp16_det
    ops.set_loss_scale("dynamic", init=2.0 ** 100)
    tr = _trainer("acc9")
    before = _snapshot(tr)
    leaked, real, si, z = _batch(0, tag="acc9")
    gi, di = G.gim_step(G.DataParallelMock(tr), leaked, real, si, z=z, micro_batches=2)
    after = _snapshot(tr)
    diff = [k for k in before if not _is_sn(k) and not torch.equal(before[k], after[k])]
    assert not diff, "a skipped accumulated step moved %s" % diff[:8]
    for opt in (tr.authenticator_opt, tr.impersonator_opt):
        st = opt.loss_scaler.state()
        assert int(opt._step_dev) == 0 and st["scale"] == 2.0 ** 99 and st["skipped"] == 1 and st["last_overflow"], st
    assert torch.isfinite(gi[0]).all() and torch.isfinite(di[0]).all()


def test_fp16_accumulated_step_at_a_usable_scale(fp16_det):
    import optimalstrategiesagainstgenerativeattacks_amd as G
    ops = fp16_det
    ops.set_loss_scale("dynamic", init=4096)
    snaps = {}
    for A in (1, 2):
        tr = _trainer("acc9")
        leaked, real, si, z = _batch(0, tag="acc9")
        G.gim_step(G.DataParallelMock(tr), leaked, real, si, z=z, **({"micro_batches": A} if A > 1 else {}))
        snaps[A] = _snapshot(tr)
        for opt in (tr.authenticator_opt, tr.impersonator_opt):
            st = opt.loss_scaler.state()
            assert (st["scale"], st["clean_steps"], st["skipped"]) == (4096.0, 1, 0) and int(opt._step_dev) == 1, (A, st)
    _assert_order_bounds("fp16, 2 micro-batches vs whole batch after one iteration", snaps[2], snaps[1])


# 10 --------------------------------------------------------------------------------------------------------------------
def _spawn(rank, world, port, out, iters, A):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    worker = os.path.join(root, "tests", "acc_dp_gpu_worker.py")
    env = dict(os.environ, GIM_DETERMINISTIC="1")
    return subprocess.Popen(["timeout", "-k", "10", "300", sys.executable, worker, str(rank), str(world), str(port), out, str(iters), TAG,
                             str(A)], env=env)


def test_ranks_times_micro_batches(tmp_path):
    """2 ranks (gloo, both on the one card) x 2 micro-batches on B = 4 - one episode per slice, total gradient scale 1 / 4, one
    all-reduce per optimizer step - against one process on the whole batch; two iterations, the "order" bounds.  Three child
    processes, each under its own time limit; the first failing status ends the test."""
    ports = iter(range(33600 + os.getpid() % 1000, 65000, 1009))
    single_out, dp_out = str(tmp_path / "single.pt"), str(tmp_path / "dp.pt")
    assert _spawn(0, 1, next(ports), single_out, 2, 1).wait() == 0, "single process on the whole batch"
    port = next(ports)
    procs = [_spawn(r, 2, port, dp_out, 2, 2) for r in range(2)]
    try:
        for r, p_ in enumerate(procs):
            assert p_.wait() == 0, "rank %d" % r
    finally:
        for p_ in procs:
            if p_.poll() is None:
                p_.kill()
                p_.wait()
    single, dp = torch.load(single_out), torch.load(dp_out)
    assert dp["adam_steps"] == single["adam_steps"] == (2, 2)
    _assert_order_bounds("2 ranks x 2 micro-batches vs single process after two iterations", dp["state"], single["state"])
    assert len(dp["outs"]) == len(single["outs"]) == 2


# 11 --------------------------------------------------------------------------------------------------------------------
def test_accumulated_iteration_needs_less_memory():
    """Default mode, 8 episodes: the peak of an iteration as 4 x 2 is strictly below the peak of the plain iteration (the ratio is a
    measurement: profiles/accumulation.txt).  Fresh trainers, the accumulated one first, one warm-up iteration each."""
    import optimalstrategiesagainstgenerativeattacks_amd as G
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    assert not ops.deterministic()
    peaks = {}
    for A in (4, 1):
        gc.collect()
        torch.cuda.empty_cache()
        tr = _trainer("acc11")
        trainer = G.DataParallelMock(tr)
        kw = {"micro_batches": A} if A > 1 else {}
        for it in range(2):
            leaked, real, si, z = _batch(it, B=8, tag="acc11")
            if it == 1:
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
            G.gim_step(trainer, leaked, real, si, z=z, **kw)
            torch.cuda.synchronize()
        peaks[A] = (torch.cuda.max_memory_allocated(), base)
        del tr, trainer, leaked, real, si, z
    (p4, b4), (p1, b1) = peaks[4], peaks[1]
    print("peak allocated, 8 episodes: 4 x 2 %.2f MiB (%.2f above the start of the iteration), plain %.2f MiB (%.2f above); "
          "ratio %.3f (above the start: %.3f)" % (p4 / 2 ** 20, (p4 - b4) / 2 ** 20, p1 / 2 ** 20, (p1 - b1) / 2 ** 20, p4 / p1,
                                                  (p4 - b4) / max(p1 - b1, 1)))
    assert p4 < p1, (p4, p1)
