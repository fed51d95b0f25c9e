"""Gradient accumulation (micro_batches), the parts that need no GPU: argument checks, the spectral-norm replay bookkeeping of
mb.SNPlan / mb.SNConv2d on stubbed launches, the factor in FusedAdam.step's signature, and the documents."""
import inspect
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gt():
    from optimalstrategiesagainstgenerativeattacks_amd import gim_img_training as gt
    return gt


class _NoTrainer:
    """Any use of the trainer is GPU work: the argument checks must come first."""

    def __getattr__(self, name):
        raise AssertionError("the step touched the trainer (%s) before it checked micro_batches" % name)


def _batch(B):
    return torch.zeros(B, 1, 1, 4, 4), torch.zeros(B, 3, 1, 4, 4), torch.zeros(B, 4, 1, 4, 4), torch.zeros(B, 3, 8)


def _step_calls(B, A):
    gt = _gt()
    leaked, real, si, z = _batch(B)
    tr = _NoTrainer()
    return [lambda: gt.gim_step(tr, leaked, real, si, z=z, micro_batches=A),
            lambda: gt.im_train_step(tr, leaked, si, z=z, micro_batches=A),
            lambda: gt.au_train_step(tr, real, real, si, micro_batches=A),
            lambda: gt.im_eval_step(tr, leaked, si, z=z, micro_batches=A),
            lambda: gt.au_eval_step(tr, real, real, si, micro_batches=A)]


def test_batch_not_divisible_by_micro_batches_raises():
    for call in _step_calls(4, 3):
        with pytest.raises(ValueError, match="cannot be cut into 3 equal micro-batches"):
            call()
    for call in _step_calls(2, 4):
        with pytest.raises(ValueError, match="equal micro-batches"):
            call()


@pytest.mark.parametrize("A", [0, -2])
def test_micro_batches_below_one_raises(A):
    for call in _step_calls(4, A):
        with pytest.raises(ValueError, match="micro_batches must be >= 1"):
            call()


@pytest.mark.parametrize("A", [2.0, "2", None, True])
def test_non_integer_micro_batches_raises(A):
    for call in _step_calls(4, A):
        with pytest.raises(ValueError, match="micro_batches must be an integer"):
            call()


def test_loops_check_micro_batches_before_anything_else():
    gt = _gt()
    with pytest.raises(ValueError, match="micro_batches"):
        gt.train_epoch(device=None, logger=None, epoch=0, trainer=_NoTrainer(), train_ds=None, val_ds=None, train_batch_size=4,
                       val_batch_size=4, num_workers=0, save_every=1, eval_every=1, save_imgs_every=1, train_eval_indices=[],
                       val_eval_indices=[], micro_batches=0)
    with pytest.raises(ValueError, match="cannot be cut into 3"):
        gt.train_epoch(device=None, logger=None, epoch=0, trainer=_NoTrainer(), train_ds=None, val_ds=None, train_batch_size=4,
                       val_batch_size=4, num_workers=0, save_every=1, eval_every=1, save_imgs_every=1, train_eval_indices=[],
                       val_eval_indices=[], micro_batches=3)
    assert inspect.signature(gt.train_gim_imgs).parameters["micro_batches"].default == 1
    for fn in (gt.gim_step, gt.im_train_step, gt.au_train_step, gt.im_eval_step, gt.au_eval_step, gt.train_epoch):
        assert inspect.signature(fn).parameters["micro_batches"].default == 1, fn.__name__


def test_slices_are_cut_like_ranks_and_merged_in_batch_order():
    gt = _gt()
    from optimalstrategiesagainstgenerativeattacks_amd import model_blocks as mb
    x = torch.arange(24.0).view(6, 4)
    sn = mb.SNReplay()
    parts = [gt._micro_batch(sn, j, 3, x, None)[1] for j in range(3)]
    assert all(p[1] is None for p in parts)
    assert torch.equal(torch.cat([p[0] for p in parts]), x) and all(p[0].shape == (2, 4) for p in parts)
    ctx, same = gt._micro_batch(sn, 0, 1, x, None)
    assert same[0] is x                       # one micro-batch: the caller's tensors, no slicing
    outs = [(p[0].mean(), p[0]) for p in parts]
    mean, cat = gt._merged(outs, cat=(1,))
    assert torch.equal(cat, x) and abs(float(mean) - float(x.mean())) < 1e-6 * float(x.mean())
    assert gt._merged(outs[:1], cat=(1,)) is outs[0]


def _stubbed_plan(launches):
    from optimalstrategiesagainstgenerativeattacks_amd import model_blocks as mb
    convs = [mb.SNConv2d(2, 3, 3, padding=1), mb.SNConv2d(3, 4, 1)]
    plan = mb.SNPlan(convs)

    def launch(rounds, training):      # what SNPlan._launch does on the host, without the kernels
        for c in plan.convs:
            c._sn_queue.clear()
        gen = plan._gen
        plan._gen += 1
        for r in range(rounds):
            out = plan._bufs.setdefault((gen & 1, r), torch.zeros(16))
            for c in plan.convs:
                c._sn_queue.append((out[0:1], out[1:4], out[4:8], (plan, gen)))
        launches.append((rounds, training))
    plan._launch = launch
    return mb, plan


def test_snplan_replay_requeues_the_same_buffers_and_keeps_gen():
    launches = []
    mb, plan = _stubbed_plan(launches)
    plan.run(2, True)                       # a plain step in front: generation 0
    assert plan._gen == 1 and launches == [(2, True)]
    sn = mb.SNReplay()
    with sn.micro_batch(0):
        plan.run(2, True)
        first = [tuple(c._sn_queue) for c in plan.convs]
        for c in plan.convs:
            c._sn_queue.clear()             # the forward pops them
        plan.run(3, True)
        second = [tuple(c._sn_queue) for c in plan.convs]
    assert plan._gen == 3 and launches == [(2, True), (2, True), (3, True)]
    assert [len(q) for q in first] == [2, 2] and [len(q) for q in second] == [3, 3]
    for j in (1, 2):
        with sn.micro_batch(j):
            plan.run(2, False)              # (the mode is micro-batch 0's: nothing is launched)
            again = [tuple(c._sn_queue) for c in plan.convs]
            plan.run(3, True)
            again2 = [tuple(c._sn_queue) for c in plan.convs]
        assert plan._gen == 3 and len(launches) == 3, "a replay launches nothing and does not advance the generation"
        for got, want in ((again, first), (again2, second)):
            for qg, qw in zip(got, want):
                assert len(qg) == len(qw)
                for tg, tw in zip(qg, qw):
                    assert all(a is b for a, b in zip(tg[:3], tw[:3])), "the same buffer objects"
                    assert tg[3][0] is plan and tg[3][1] == tw[3][1], "the original (plan, generation) guard"
        assert again[0][0][3][1] == 1 and again2[0][0][3][1] == 2
        assert not plan.stale(1) and not plan.stale(2)
    # outside an accumulated step, and in the next one, the plan launches again
    plan.run(2, True)
    assert plan._gen == 4 and len(launches) == 4
    with mb.SNReplay().micro_batch(0):
        plan.run(2, True)
    assert plan._gen == 5 and len(launches) == 5


def test_snplan_replay_refuses_a_call_micro_batch_zero_did_not_make():
    launches = []
    mb, plan = _stubbed_plan(launches)
    sn = mb.SNReplay()
    with sn.micro_batch(0):
        plan.run(2, True)
    with sn.micro_batch(1):
        plan.run(2, True)
        with pytest.raises(RuntimeError, match="micro-batch 0"):
            plan.run(3, True)
    with sn.micro_batch(2):
        with pytest.raises(RuntimeError, match="micro-batch 0"):
            plan.run(3, True)               # other rounds than recorded
    assert mb._SN_REPLAY[0] is None, "the context is left behind on an exception too"
    assert len(launches) == 1


def test_conv_without_plan_replays_its_own_power_iteration(monkeypatch):
    from optimalstrategiesagainstgenerativeattacks_amd import model_blocks as mb
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    conv = mb.SNConv2d(2, 3, 1)
    made, used = [], []

    def sigma(w, u, v, training):
        made.append((torch.ones(1) * len(made), torch.zeros(3), torch.zeros(2)))
        return made[-1]
    monkeypatch.setattr(ops, "spectral_sigma", sigma)
    monkeypatch.setattr(ops, "conv2d", lambda x, w, b, res, s, u_s, v_s, *a: used.append((s, u_s, v_s)))
    sn = mb.SNReplay()
    for j in range(3):
        with sn.micro_batch(j):
            conv(None)
            conv(None)
    assert len(made) == 2, "two calls per micro-batch: two power iterations per accumulated step"
    for j in range(3):
        for c in range(2):
            assert all(a is b for a, b in zip(used[2 * j + c], made[c]))
    conv(None)
    assert len(made) == 3, "a plain call runs its own"


def test_adam_step_takes_the_micro_batch_factor_and_baselines_do_not():
    from optimalstrategiesagainstgenerativeattacks_amd import baseline_training as bt
    from optimalstrategiesagainstgenerativeattacks_amd import optim
    assert inspect.signature(optim.FusedAdam.step).parameters["micro_batches"].default == 1
    # BatchNorm statistics span the whole batch: slices in sequence cannot supply them, so the baseline trainers refuse the argument
    for cls in (bt.SiameseTrainer, bt.ArcFaceTrainer):
        for name in ("__init__", "train_step"):
            sig = inspect.signature(getattr(cls, name))
            assert "micro_batches" not in sig.parameters
            assert not any(p.kind is inspect.Parameter.VAR_KEYWORD for p in sig.parameters.values()), (cls.__name__, name)


def test_documents_mention_micro_batches():
    for name, needles in (("README.md", ("micro_batches",)), ("DESIGN.md", ("micro_batches", "Accumulated steps")),
                          ("INTEGRATION.md", ("micro_batches",))):
        with open(os.path.join(ROOT, name)) as f:
            text = f.read()
        for needle in needles:
            assert needle in text, (name, needle)
