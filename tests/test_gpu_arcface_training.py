"""Training the ArcFace baseline on the GPU (baseline_training.py) against what the REFERENCE's model gave when torch trained it on
the CPU (tests/golden/arcface_train.npz, written by tools/make_arcface_train_golden.py; weights, images and the synthetic bank are
regenerated from names by tests/baseline_fill.py, tests/arcface_fill.py and tests/siamese_fill.py), then the round trip train ->
checkpoint -> resume -> authentication evaluation.  Every test is a single shot."""
import csv
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import arcface_fill as af
from tests import baseline_fill as bf
from tests import siamese_fill as sf
from tests.helpers import filled_sd, load_keys, load_npz, relerr

BLOCK = 1e-4        # emb, logits, loss, gradients against the reference
STATS = 3e-5        # running statistics (one operator)

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _model(tag, n_classes, drop=0.0):
    from optimalstrategiesagainstgenerativeattacks_amd import baselines as bl
    model = bl.ArcFace(bl.Backbone(af.NUM_LAYERS, drop, 'ir_se', af.IMG_SIZE, af.IMG_CHANNELS), af.EMB_DIM, n_classes)
    model.load_state_dict(bf.filled_state(af.keys(n_classes), tag, torch.float32), strict=True)
    return model.to(dev())


def _at(t, idx):
    return t.detach().reshape(-1)[torch.from_numpy(idx).to(t.device)].double().cpu()


def test_protocol_vs_reference_golden():
    """Three Adam iterations (lr = 1e-5) at B = 8 from a conditioned state.  emb, logits and loss of every iteration at
    max(3 x the reference's own fp32-vs-fp64 deviation, 1e-4); five BatchNorms' running statistics at max(3 x floor, 3e-5); the
    iteration-0 gradient samples of every non-small tensor at max(3 x floor, 1e-4); every small tensor's whole norm <= 1e-5 of the
    largest gradient norm; and the first update: |dp - dp_ref| <= 0.1 lr on the sampled elements with |g_ref| >= 1e-3 rms(g) (fp32
    rounding of a parameter of magnitude <= 2 is 0.012 lr, a wrong sign costs 2 lr, a missed update lr).

    Measured on MI355X: gradients <= 4.0e-6, first update within 1.9e-8.  In two of seven processes - each the first GPU process on a
    freshly started machine - the gradients from body.18.res_layer.0 towards the input were off instead (dbeta 2.2e-3, dgamma 1.3e-3
    there, 3e-4 .. 6e-4 upstream, the same figures both times) with emb, logits, loss and the gradients of body.23 .. body.18.res_layer.1
    right; the cause is not found, the bounds stay."""
    from optimalstrategiesagainstgenerativeattacks_amd.baseline_training import ArcFaceTrainer
    gold = load_npz("arcface_train.npz")
    model = _model(af.PROTO_TAG, af.PROTO_CLASSES)
    tr = ArcFaceTrainer(model, lr=af.PROTO_LR)
    label = torch.from_numpy(af.proto_labels()).to(dev())
    names = [k for k, _ in model.named_parameters()]
    assert names == list(gold["grad_names"]) == [k for k, _ in af.parameter_entries()]
    small = set(gold["small"].tolist())
    g_ref, d_ref = af.unpack(gold["grad"]), af.unpack(gold["delta"], af.delta_index)
    norms, floors = dict(zip(names, gold["gradnorm"])), dict(zip(names, gold["floor_grad"]))
    largest = max(norms.values())
    errs, bounds = {}, {}
    for it in range(af.PROTO_ITERS):
        x = torch.from_numpy(af.proto_images(it)).float().to(dev())
        if it == 0:
            before = {k: _at(p, af.delta_index(p.numel())) for k, p in model.named_parameters()}
        loss, acc = tr.train_step(x, label, it)
        for nm, got in (("emb", tr.last_emb), ("logits", tr.last_logits), ("loss", loss)):
            key = "it%d/%s" % (it, nm)
            errs[key], bounds[key] = relerr(got, gold[key]), max(3.0 * float(gold["floor/" + key]), BLOCK)
        sd = model.state_dict()
        for bn in af.RUNNING:
            for leaf in ("running_mean", "running_var"):
                key = "it%d/run/%s.%s" % (it, bn, leaf)
                errs[key], bounds[key] = relerr(sd["emb_model.%s.%s" % (bn, leaf)], gold[key]), max(3.0 * float(gold["floor/" + key]), STATS)
            assert int(sd["emb_model.%s.num_batches_tracked" % bn]) == 7 + it + 1
        if it == 0:
            worst_update, masked, total = 0.0, 0, 0
            for k, p in model.named_parameters():
                if k in small:
                    e = float(p.grad.double().norm()) / largest
                    print("grad/%s (small): %.2e of the largest gradient norm" % (k, e))
                    assert e <= 1e-5, (k, e)
                    continue
                errs["grad/" + k] = relerr(_at(p.grad, af.sample_index(p.numel())), g_ref[k])
                bounds["grad/" + k] = max(3.0 * float(floors[k]), BLOCK)
                gr = torch.from_numpy(g_ref[k][::2]).double()
                keep = gr.abs() >= af.MASK_REL * float(norms[k]) / math.sqrt(p.numel())
                d = (_at(p, af.delta_index(p.numel())) - before[k] - torch.from_numpy(d_ref[k]).double()).abs()[keep]
                masked, total = masked + int((~keep).sum()), total + keep.numel()
                if d.numel() and float(d.max()) > 0.1 * af.PROTO_LR:
                    print("update of %s: |dp - dp_ref| up to %.3e" % (k, float(d.max())))
                worst_update = max(worst_update, float(d.max()) if d.numel() else 0.0)
            print("first update: worst |dp - dp_ref| %.3e (0.1 lr = %.1e); %d of %d sampled elements masked" % (worst_update, 0.1 * af.PROTO_LR, masked, total))
    worst = sorted(((e / bounds[k], k) for k, e in errs.items()), reverse=True)[:12]
    for _, k in worst:
        print("%-60s %.3e  (bound %.3e)" % (k, errs[k], bounds[k]))
    over = [k for k in errs if errs[k] >= bounds[k]]
    if over:        # in the order of the backward pass, last layer first
        print("over their bounds: " + ", ".join("%s %.1e" % (k, errs[k]) for k in reversed(over)))
    for k, e in errs.items():
        assert e < bounds[k], (k, e, bounds[k])
    assert worst_update <= 0.1 * af.PROTO_LR, worst_update


def _bank(per_class=sf.BANK_PER_CLASS, m=1, n=1, k=1, mirror=True):
    import optimalstrategiesagainstgenerativeattacks_amd as G
    imgs, offs = sf.separable_bank(per_class=per_class)
    return imgs, G.EpisodeBank(torch.from_numpy(imgs).to(dev()), offs, m, n, k, example_cnt_per_class=1, mirror=mirror, seed=5)


def test_loss_curve_vs_reference_golden():
    """24 iterations at B = 16, lr = 1e-4 on the synthetic separable bank, drawn by IdentitySampler (the fixture stores what the tool
    drew): every 8-iteration window mean of the loss within max(3 x the reference's own fp32-vs-fp64 deviation, 1e-2) of the
    reference's fp64 curve, of the accuracy within max(3 x stored, 1 / 16)."""
    from optimalstrategiesagainstgenerativeattacks_amd.baseline_training import ArcFaceTrainer, IdentitySampler
    gold = load_npz("arcface_train.npz")
    imgs, bank = _bank()
    sampler = IdentitySampler(bank, af.CURVE_B, af.CURVE_SEED)
    tr = ArcFaceTrainer(_model(af.CURVE_TAG, af.CURVE_CLASSES), lr=af.CURVE_LR)
    out = []
    for it in range(af.CURVE_ITERS):
        idx, flip, label = sampler.draw(it)
        assert np.array_equal(idx, gold["curve/idx"][it]) and np.array_equal(flip, gold["curve/flip"][it]) and np.array_equal(label, gold["curve/label"][it]), it
        x, lab = sampler.batch(it)
        if it == 0:     # the images the reference was trained on
            assert torch.equal(x.cpu(), torch.from_numpy(sf.gather_host(imgs, idx, flip))) and torch.equal(lab.cpu(), torch.from_numpy(label))
        out.extend(tr.train_step(x, lab, it))
    curve = torch.stack(out).double().cpu().numpy().reshape(af.CURVE_ITERS, 2)
    loss, acc = curve[:, 0], curve[:, 1]
    print("loss     ", np.round(loss, 4).tolist())
    print("reference", np.round(gold["curve/loss"], 4).tolist())
    print("acc      ", acc.tolist())
    print("reference", gold["curve/acc"].tolist())
    for nm, got, ref, env, floor in (("loss", loss, gold["curve/loss"], gold["curve/env_loss"], 1e-2),
                                     ("acc", acc, gold["curve/acc"], gold["curve/env_acc"], 1.0 / 16)):
        d = np.abs(sf.window_means(got, af.WINDOW) - sf.window_means(ref, af.WINDOW))
        bound = np.maximum(3.0 * env, floor)
        print("%s window means: largest deviation %.3e (bound there %.3e)" % (nm, d.max(), bound[d.argmax()]))
        assert (d <= bound).all(), (nm, d.tolist(), bound.tolist())


def test_state_dict_round_trip_and_inference_path():
    """After two steps the trainer's state dict has the reference's keys, shapes and order and loads strict=True into a fresh
    baselines.ArcFace; the inference path (derived parameters, no training code) is finite on it, was dropped by the training
    steps, and gives bit-equal embeddings before and after the round trip."""
    from optimalstrategiesagainstgenerativeattacks_amd import baselines as bl
    from optimalstrategiesagainstgenerativeattacks_amd.baseline_training import ArcFaceTrainer
    model = _model(af.PROTO_TAG, af.PROTO_CLASSES).train(mode=False)
    x = torch.from_numpy(af.proto_images(0)).float().to(dev())
    label = torch.from_numpy(af.proto_labels()).to(dev())
    with torch.no_grad():
        before = model(x).clone()
    assert model.emb_model._derived is not None
    tr = ArcFaceTrainer(model, lr=1e-4)
    for it in range(2):
        tr.train_step(x, label, it)
    assert model.emb_model._derived is None and not model.training
    sd = tr.state_dict()["model"]
    assert [[k, list(v.shape)] for k, v in sd.items()] == [[k, s] for k, s, _ in af.keys()]
    assert all(not v.is_cuda for v in sd.values())
    with torch.no_grad():
        after = model(x)
    assert torch.isfinite(after).all() and relerr(after, before) > 1e-4
    assert relerr(after.norm(dim=1), torch.ones(af.PROTO_B)) < 1e-6
    fresh = bl.ArcFace(bl.Backbone(af.NUM_LAYERS, 0.0, 'ir_se', af.IMG_SIZE, af.IMG_CHANNELS), af.EMB_DIM, af.PROTO_CLASSES)
    fresh.load_state_dict(sd, strict=True)
    with torch.no_grad():
        assert torch.equal(fresh.to(dev()).train(mode=False)(x), after)
    with pytest.raises(NotImplementedError):
        model(x, label)       # the inference class keeps refusing labels: training is arcface_forward_train


def test_fp16_path_and_bad_arguments_are_refused():
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    from optimalstrategiesagainstgenerativeattacks_amd.baseline_training import ArcFaceTrainer, arcface_forward_train
    model = _model(af.PROTO_TAG, af.PROTO_CLASSES, drop=0.6)
    x = torch.from_numpy(af.proto_images(0)).float().to(dev())
    label = torch.from_numpy(af.proto_labels()).to(dev())
    prev = ops.set_matrix_path("fp16")
    try:
        with pytest.raises(RuntimeError, match="fp32 matrix path only"):
            ArcFaceTrainer(model).train_step(x, label, 0)
    finally:
        ops.set_matrix_path(prev)
    with pytest.raises(RuntimeError, match="dropout="):
        arcface_forward_train(model, x, label)
    with pytest.raises(RuntimeError, match="int64"):
        arcface_forward_train(model, x, label.int(), (0, 0))
    with pytest.raises(RuntimeError, match="at least two"):
        arcface_forward_train(model, x[:1], label[:1], (0, 0))
    with pytest.raises(TypeError):
        ArcFaceTrainer(model.emb_model)


def test_train_resume_and_authentication_table(tmp_path):
    """train_arcface (drop_ratio 0.6) for 8 iterations with a checkpoint every 3; a second run stopped at 6 and resumed to 8
    reproduces the first one's iterations 7 and 8 bit for bit (deterministic mode: no float atomics in the convolutions' weight
    gradients either; the dropout masks are keyed by the iteration); get_arcface_authenticator loads the checkpoint;
    eval_authentication_task writes its six rows with the trained baseline."""
    import optimalstrategiesagainstgenerativeattacks_amd as G
    from optimalstrategiesagainstgenerativeattacks_amd import authentication_eval as ae
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    m, n, k, bs = 1, 3, 4, 4
    _, bank = _bank(per_class=10, m=m, n=n, k=k, mirror=False)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    kw = dict(batch_size=8, lr=1e-4, drop_ratio=0.6, log_every=1, save_every=3, seed=4)
    prev = ops.set_deterministic(True)
    try:
        log_a = G.Logger(log_dir=str(tmp_path / "logs_a"), img_dir=str(tmp_path / "imgs_a"))
        G.train_arcface(dev(), bank, a, 8, logger=log_a, **kw)
        G.train_arcface(dev(), bank, b, 6, **kw)
        log_b = G.Logger(log_dir=str(tmp_path / "logs_b"), img_dir=str(tmp_path / "imgs_b"))
        G.train_arcface(dev(), bank, b, 8, logger=log_b, **kw)
    finally:
        ops.set_deterministic(prev)
    la, lb = dict(log_a.stats["arcface"]["loss"]), dict(log_b.stats["arcface"]["loss"])
    assert sorted(la) == list(range(1, 9)) and sorted(lb) == [7, 8]
    assert la[7] == lb[7] and la[8] == lb[8] and all(np.isfinite(v) and v > 0 for v in la.values())
    assert sorted(os.listdir(os.path.join(a, "ckpts"))) == ["model_%08d.pt" % s for s in (3, 6, 8)]
    assert sorted(os.listdir(os.path.join(b, "ckpts"))) == ["model_%08d.pt" % s for s in (3, 6, 8)]
    args = json.load(open(os.path.join(a, "args.json")))
    assert {kk: args[kk] for kk in ("img_size", "img_channels", "num_layers", "dropout", "emb_dim", "th")} == \
        {"img_size": 32, "img_channels": 1, "num_layers": 50, "dropout": 0.6, "emb_dim": 512, "th": 1.5}
    ck_a, ck_b = (torch.load(os.path.join(d, "ckpts", "model_00000008.pt"), map_location="cpu") for d in (a, b))
    assert ck_a["global_step"] == ck_b["global_step"] == 8 and set(ck_a) == {"arcface", "opt", "global_step"}
    assert [kk for kk in ck_a["arcface"]] == [e[0] for e in af.keys()] and ck_a["arcface"]["head.kernel"].shape == (512, 8)
    for kk, v in ck_a["arcface"].items():
        assert torch.equal(v, ck_b["arcface"][kk]), kk
    mid = torch.load(os.path.join(b, "ckpts", "model_00000006.pt"), map_location="cpu")["arcface"]
    assert not torch.equal(mid["head.kernel"], ck_b["arcface"]["head.kernel"])

    # the checkpoint as the evaluation loads it
    path, args = ae.get_exp_args_from_dir(a, "ckpts")
    assert path.endswith("model_00000008.pt")
    au = ae.get_arcface_authenticator(dev(), path, args)
    batch = bank.batch([0, 1, 2, 3])
    out, _ = au.act(test_sample=batch["real_sample"][:, :1], si_sample=batch["si_sample"][:, :1])
    assert torch.isfinite(out).all() and float(out.max()) <= 0.0

    # the result table with the trained baseline (the tiny GIM experiment directory of tests/test_gpu_baselines.py's end-to-end test)
    keys = load_keys("32_1_512")
    gim = tmp_path / "gim"
    (gim / "ckpts").mkdir(parents=True)
    torch.save({"authenticator": filled_sd(keys["au"], "e2e/au/", torch.float32), "impersonator": filled_sd(keys["im"], "e2e/im/", torch.float32)},
               str(gim / "ckpts" / "model_00000003.pt"))
    (gim / "args.json").write_text(json.dumps({"target_img_size": 32, "img_channels": 1, "style_dim": 512, "use_img_att": False,
                                               "num_env_noise_layers": 4, "remove_noise_mean": True}))
    bank.root = "synthetic"
    table = str(tmp_path / "out" / "arcface.csv")
    ae.eval_authentication_task(dev(), bank, m, n, k, bs, 0, str(gim), table, baseline_exp_dir=a, baseline_type="arcface")
    with open(table) as f:
        rows = list(csv.DictReader(f))
    assert [(r["au_type"], r["im_type"]) for r in rows] == [(x, i) for x in ("gim", "arcface") for i in ("gim", "replay", "rnd_src")]
    for r in rows:
        for col in ("acc", "acc_on_fake", "acc_on_real", "auc"):
            assert 0.0 <= float(r[col]) <= 1.0, r
