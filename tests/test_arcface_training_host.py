"""Host side of the ArcFace baseline's training (baseline_training.py): the identity sampler, argument validation, the parameter
order of the trainer, the library's new entry points, the CPU refusals and the fixture's own conditions.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

from tests import arcface_fill as af
from tests import siamese_fill as sf
from tests.helpers import load_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ("gim_bn_apply_fwd", "gim_bn_bwd_reduce", "gim_bn_bwd_dx", "gim_prelu_fwd", "gim_prelu_bwd", "gim_se_tail_bwd",
               "gim_subsample2_fwd", "gim_subsample2_bwd", "gim_dropout", "gim_l2norm_rows_bwd", "gim_col_l2norm_fwd", "gim_col_l2norm_bwd",
               "gim_arcface_margin_fwd", "gim_arcface_margin_bwd", "gim_softmax_ce_fwd", "gim_softmax_ce_bwd")


class _Bank:
    """What IdentitySampler and train_arcface's argument checks read of a bank."""

    def __init__(self, sizes, mirror=True, S=32, C=1):
        self.offsets = np.concatenate([[0], np.cumsum(sizes)])
        self.mirror, self.S, self.C = mirror, S, C


def test_identity_sampler_contract():
    from optimalstrategiesagainstgenerativeattacks_amd.baseline_training import IdentitySampler
    sizes = [3, 1, 7, 0, 2, 5]       # ragged, one empty class
    bank = _Bank(sizes)
    s = IdentitySampler(bank, 64, seed=9)
    assert s.n_classes == 6
    seen_flip, seen_cls = set(), set()
    for it in range(20):
        idx, flip, label = s.draw(it)
        assert idx.dtype == np.int32 and flip.dtype == np.uint8 and label.dtype == np.int64 and idx.shape == flip.shape == label.shape == (64,)
        assert ((idx >= bank.offsets[label]) & (idx < bank.offsets[label + 1])).all()       # every index lies in its label's class
        assert (label != 3).all()
        seen_flip |= set(flip.tolist())
        seen_cls |= set(label.tolist())
    assert seen_flip == {0, 1} and seen_cls == {0, 1, 2, 4, 5}
    # a function of (seed, it) only: a fresh sampler, any call order
    t = IdentitySampler(_Bank(sizes), 64, seed=9)
    for it in (7, 0, 7):
        for u, v in zip(s.draw(it), t.draw(it)):
            assert np.array_equal(u, v)
    assert not np.array_equal(s.draw(1)[0], s.draw(2)[0])
    assert not np.array_equal(s.draw(1)[0], IdentitySampler(_Bank(sizes), 64, seed=10).draw(1)[0])
    # uniform over classes, then uniform within the class: the single image of class 1 is drawn about as often as all of class 2
    idx = np.concatenate([IdentitySampler(_Bank(sizes), 64, seed=1).draw(it)[0] for it in range(200)])
    share_1, share_2 = np.mean(idx == 3), np.mean((idx >= 4) & (idx < 11))
    assert abs(share_1 - 0.2) < 0.02 and abs(share_2 - 0.2) < 0.02
    # no flips without mirror
    assert not IdentitySampler(_Bank(sizes, mirror=False), 64, seed=9).draw(3)[1].any()
    with pytest.raises(ValueError):
        IdentitySampler(_Bank(sizes), 1)
    with pytest.raises(ValueError):
        IdentitySampler(_Bank([0, 0]), 8)


def test_train_arcface_validates_its_arguments(tmp_path):
    from optimalstrategiesagainstgenerativeattacks_amd.baseline_training import train_arcface
    ok = _Bank([4, 4, 4])
    for bank, kw in ((ok, dict(num_layers=34)), (_Bank([4, 4], S=48), {}), (ok, dict(drop_ratio=1.0)), (ok, dict(drop_ratio=-0.1)),
                     (ok, dict(batch_size=1)), (_Bank([8]), {})):
        with pytest.raises(ValueError):
            train_arcface("cpu", bank, str(tmp_path / "x"), 1, **kw)
    with pytest.raises(ValueError):
        train_arcface("cpu", ok, str(tmp_path / "x"), -1)
    with pytest.raises(ValueError, match="seed"):
        train_arcface("cpu", ok, str(tmp_path / "x"), 1, seed=-1)
    assert not os.path.exists(str(tmp_path / "x"))      # refused before anything is written


def _expected_parameter_names(num_layers):
    from optimalstrategiesagainstgenerativeattacks_amd.baselines import unit_plan
    names = ["input_layer.0.weight", "input_layer.1.weight", "input_layer.1.bias", "input_layer.2.weight",
             "output_layer.0.weight", "output_layer.0.bias", "output_layer.3.weight", "output_layer.3.bias",
             "output_layer.4.weight", "output_layer.4.bias"]
    for i, (cin, depth, _) in enumerate(unit_plan(num_layers)):
        u = "body.%d." % i
        if cin != depth:
            names += [u + "shortcut_layer.0.weight", u + "shortcut_layer.1.weight", u + "shortcut_layer.1.bias"]
        names += [u + "res_layer." + leaf for leaf in ("0.weight", "0.bias", "1.weight", "2.weight", "3.weight", "4.weight", "4.bias",
                                                        "5.fc1.weight", "5.fc2.weight")]
    return ["emb_model." + n for n in names] + ["head.kernel"]


@pytest.mark.parametrize("num_layers", [50, 100, 152])
def test_trainer_parameter_order_is_the_references(num_layers):
    from optimalstrategiesagainstgenerativeattacks_amd import baselines as bl
    from optimalstrategiesagainstgenerativeattacks_amd.baseline_training import ArcFaceTrainer
    model = bl.ArcFace(bl.Backbone(num_layers, 0.6, 'ir_se', 32, 1), 512, 11)
    names = [k for k, _ in model.named_parameters()]
    assert names == _expected_parameter_names(num_layers)
    if num_layers == 50:        # the key list recorded from the reference's own model
        assert names == [k for k, _ in af.parameter_entries()]
        tr = ArcFaceTrainer(model)
        params = tr.opt.param_groups[0]["params"]
        assert len(tr.opt.param_groups) == 1 and [p.shape for p in params] == [p.shape for p in model.parameters()]
        assert params[-1].shape == (512, 11) and tr.opt.param_groups[0]["lr"] == 1e-4
        with pytest.raises(TypeError):
            ArcFaceTrainer(model.emb_model)


def test_new_entry_points_are_declared_bound_and_exported():
    import optimalstrategiesagainstgenerativeattacks_amd as G
    from optimalstrategiesagainstgenerativeattacks_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "gim_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.SIGNATURES, name
    csrc = os.path.join(ROOT, "optimalstrategiesagainstgenerativeattacks_amd", "csrc")
    src = open(os.path.join(csrc, "irse_train.hip")).read()
    assert "atomic" not in src.replace("float atomics", "") and "hipMalloc" not in src and "getenv" not in src
    assert "irse_train.hip" in open(os.path.join(csrc, "Makefile")).read()
    for name in ("IdentitySampler", "ArcFaceTrainer", "arcface_forward_train", "margin_softmax_loss", "top1_accuracy", "train_arcface"):
        assert name in G.__all__ and hasattr(G, name), name
    for fn in ("BatchNormFn", "PReLUFn", "SETailFn", "Subsample2Fn", "DropoutFn", "L2NormRowsFn", "ColL2NormFn", "ArcMarginFn", "SoftmaxCEFn",
               "batch_norm", "prelu", "se_tail_train", "subsample2", "dropout", "l2norm_rows_train", "col_l2norm", "arc_margin", "softmax_ce"):
        assert hasattr(ops, fn), fn


def test_entry_points_check_their_arguments_before_any_launch():
    """NULL pointers only (as tests/test_siamese_training_host.py does): a call is refused on the host, and if a check ever regressed
    there would be no address for a kernel to touch."""
    import __graft_entry__
    from optimalstrategiesagainstgenerativeattacks_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        __graft_entry__.build()
    lib = _lib.load()
    n = None
    for name, call in (
            ("bn_apply_fwd", lambda: lib.gim_bn_apply_fwd(n, n, n, n, n, n, n, 16, 8, n)),
            ("bn_bwd_reduce", lambda: lib.gim_bn_bwd_reduce(n, n, n, n, n, n, n, n, n, n, n, n, n, n, 16, 8, n)),
            ("bn_bwd_dx", lambda: lib.gim_bn_bwd_dx(n, n, n, n, n, n, n, n, n, n, 16, 8, n)),
            ("prelu_fwd", lambda: lib.gim_prelu_fwd(n, n, n, 16, 8, n)),
            ("prelu_bwd", lambda: lib.gim_prelu_bwd(n, n, n, n, n, n, n, 16, 8, n)),
            ("se_tail_bwd", lambda: lib.gim_se_tail_bwd(n, n, n, n, n, 2, 2, 2, 8, n)),
            ("subsample2_fwd", lambda: lib.gim_subsample2_fwd(n, n, 1, 4, 4, 8, n)),
            ("subsample2_bwd", lambda: lib.gim_subsample2_bwd(n, n, 1, 4, 4, 8, n)),
            ("dropout", lambda: lib.gim_dropout(n, n, 16, 0.5, 0, 0, n)),
            ("l2norm_rows_bwd", lambda: lib.gim_l2norm_rows_bwd(n, n, n, 2, 8, n)),
            ("col_l2norm_fwd", lambda: lib.gim_col_l2norm_fwd(n, n, 4, 4, n)),
            ("col_l2norm_bwd", lambda: lib.gim_col_l2norm_bwd(n, n, n, 4, 4, n)),
            ("arcface_margin_fwd", lambda: lib.gim_arcface_margin_fwd(n, n, n, 2, 4, 64.0, 0.9, 0.5, 0.2, -0.9, n)),
            ("arcface_margin_bwd", lambda: lib.gim_arcface_margin_bwd(n, n, n, n, 2, 4, 64.0, 0.9, 0.5, 0.2, -0.9, n)),
            ("softmax_ce_fwd", lambda: lib.gim_softmax_ce_fwd(n, n, n, n, n, 2, 4, n)),
            ("softmax_ce_bwd", lambda: lib.gim_softmax_ce_bwd(n, n, n, n, n, 2, 4, n))):
        assert call() < 0, name
        assert name.encode() in lib.gim_last_error(), (name, lib.gim_last_error())


def test_cpu_tensors_are_refused():
    from optimalstrategiesagainstgenerativeattacks_amd import baselines as bl
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    from optimalstrategiesagainstgenerativeattacks_amd.baseline_training import arcface_forward_train
    z, v, lab = torch.zeros(2, 2, 2, 4), torch.zeros(4), torch.zeros(2, dtype=torch.int64)
    for call in (lambda: ops.batch_norm(z, v, v, v.clone(), v.clone(), None), lambda: ops.prelu(z, v), lambda: ops.subsample2(z),
                 lambda: ops.se_tail_train(z, torch.zeros(2, 4), z), lambda: ops.dropout(z, 0.5, 0), lambda: ops.l2norm_rows_train(torch.zeros(2, 4)),
                 lambda: ops.col_l2norm(torch.zeros(4, 3)), lambda: ops.arc_margin(torch.zeros(2, 3), lab), lambda: ops.softmax_ce(torch.zeros(2, 3), lab)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    model = bl.ArcFace(bl.Backbone(50, 0.0, 'ir_se', 32, 1), 512, 11)
    with pytest.raises(RuntimeError, match="no CPU path"):
        arcface_forward_train(model, torch.zeros(2, 1, 32, 32), lab)


def test_fixture_conditions():
    """The conditions tools/make_arcface_train_golden.py asserts on the reference alone, re-checked from the stored floors."""
    g = load_npz("arcface_train.npz")
    assert os.path.getsize(os.path.join(af.GOLDEN, "arcface_train.npz")) < (1 << 20)
    entries = af.parameter_entries()
    names = [k for k, _ in entries]
    assert len(names) == 236 and names == g["grad_names"].tolist() and sum(n for _, n in entries) > 30e6
    for it in range(af.PROTO_ITERS):
        for nm, shape in (("emb", (af.PROTO_B, af.EMB_DIM)), ("logits", (af.PROTO_B, af.PROTO_CLASSES)), ("loss", ())):
            key = "it%d/%s" % (it, nm)
            assert g[key].shape == shape and np.isfinite(g[key]).all() and 0.0 <= float(g["floor/" + key]) <= 3e-5, key
        logits, label = g["it%d/logits" % it], af.proto_labels()
        lse = np.log(np.exp(logits - logits.max(1, keepdims=True)).sum(1)) + logits.max(1)
        assert abs((lse - logits[np.arange(af.PROTO_B), label]).mean() - float(g["it%d/loss" % it])) < 1e-9
        assert np.allclose(np.linalg.norm(g["it%d/emb" % it].astype(np.float64), axis=1), 1.0, atol=1e-6)
        for bn in af.RUNNING:
            for leaf in ("running_mean", "running_var"):
                key = "it%d/run/%s.%s" % (it, bn, leaf)
                assert g[key].ndim == 1 and np.isfinite(g[key]).all() and 0.0 <= float(g["floor/" + key]) < 1e-4, key
    small = g["small"].tolist()
    assert len(small) <= 10 and set(small) <= set(names)
    norms, floors = dict(zip(names, g["gradnorm"])), dict(zip(names, g["floor_grad"]))
    largest = max(norms.values())
    for k in names:
        assert (norms[k] < af.SMALL_REL * largest) == (k in small), k
        if k not in small:
            assert 0.0 <= floors[k] <= 3e-5, (k, floors[k])
    g_ref, d_ref = af.unpack(g["grad"]), af.unpack(g["delta"], af.delta_index)
    masked = total = 0
    for k, numel in entries:
        assert len(g_ref[k]) == min(numel, af.SAMPLES) and len(d_ref[k]) == len(af.delta_index(numel))
        if k in small:
            continue
        keep = np.abs(g_ref[k][::2]) >= af.MASK_REL * norms[k] / np.sqrt(numel)
        masked, total = masked + int((~keep).sum()), total + len(keep)
        # the first Adam step is -lr * sign(g) wherever the gradient is well above the optimizer's eps
        assert np.allclose(d_ref[k][keep], -af.PROTO_LR * np.sign(g_ref[k][::2][keep]), rtol=0, atol=0.01 * af.PROTO_LR), k
    assert masked / total <= 0.05 and abs(masked / total - float(g["masked_share"])) < 1e-12
    assert float(g["worst_update_f32"]) <= 0.1 * af.PROTO_LR
    # units
    for cin, depth, stride, body_idx in af.UNITS:
        name = af.unit_name(cin, depth, stride)
        x, dy = af.unit_input(cin, depth, stride)
        assert g[name + "/out"].shape == dy.shape and g[name + "/dx"].shape == x.shape
        ent, pre = af.unit_entries(body_idx)
        for k, s, kind in ent:
            leaf = k[len(pre):]
            if kind.startswith("bn.running"):
                assert g["%s/run/%s" % (name, leaf)].shape == tuple(s) and float(g["floor/%s/run/%s" % (name, leaf)]) < 1e-4
            elif kind != "bn.num_batches_tracked":
                assert len(g["%s/grad/%s" % (name, leaf)]) == min(int(np.prod(s)), af.SAMPLES) and float(g["%s/gradnorm/%s" % (name, leaf)]) >= 0
                assert float(g["floor/%s/grad/%s" % (name, leaf)]) <= 3e-5 or float(g["%s/gradnorm/%s" % (name, leaf)]) < 1e-9
        for leaf in ("out", "dx"):
            assert float(g["floor/%s/%s" % (name, leaf)]) <= 3e-5
    # curve: what the sampler draws today is what the tool drew
    from optimalstrategiesagainstgenerativeattacks_amd.baseline_training import IdentitySampler
    imgs, offs = sf.separable_bank()
    sampler = IdentitySampler(_Bank(np.diff(offs)), af.CURVE_B, af.CURVE_SEED)
    for it in range(af.CURVE_ITERS):
        for u, key in zip(sampler.draw(it), ("idx", "flip", "label")):
            assert np.array_equal(u, g["curve/" + key][it]), (it, key)
    n_win = af.CURVE_ITERS - af.WINDOW + 1
    for nm in ("loss", "acc"):
        assert g["curve/" + nm].shape == g["curve/%s_f32" % nm].shape == (af.CURVE_ITERS,) and g["curve/env_" + nm].shape == (n_win,)
        assert np.allclose(g["curve/env_" + nm], np.abs(sf.window_means(g["curve/%s_f32" % nm], af.WINDOW) - sf.window_means(g["curve/" + nm], af.WINDOW)), atol=1e-15)
    first = sf.window_means(g["curve/loss"], af.WINDOW)[0]
    assert g["curve/env_loss"].max() <= 0.01 * first
    assert sf.window_means(g["curve/loss"], af.WINDOW)[-1] < 0.05 * first and g["curve/acc"][-6:].min() == 1.0      # the net learns the bank
