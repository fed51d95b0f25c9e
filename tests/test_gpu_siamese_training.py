"""Training the siamese baseline on the GPU (baseline_training.py) against what the REFERENCE's model gave when torch trained it on
the CPU (tests/golden/siamese_train.npz, written by tools/make_siamese_train_golden.py; weights, images and the synthetic bank are
regenerated from names by tests/baseline_fill.py and tests/siamese_fill.py), then the round trip train -> checkpoint -> resume ->
authentication evaluation.  Every test is a single shot."""
import csv
import json
import os

import numpy as np
import pytest
import torch

from tests import baseline_fill as bf
from tests import siamese_fill as sf
from tests.helpers import GOLDEN, filled_sd, load_keys, load_npz, relerr, relerr_floor

PARITY = 1e-3       # the project's parity contract against the reference (test_trainer_protocol_vs_reference_golden)

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _keys():
    with open(os.path.join(GOLDEN, "baseline_keys.json")) as f:
        return json.load(f)["keys"][sf.CFG]


def _model(tag):
    from optimalstrategiesagainstgenerativeattacks_amd import baselines as bl
    enc = bl.ProtonetEmbeddingNet(1, 32)
    model = bl.SiameseNet(enc, enc.embedding_dim)
    model.load_state_dict(bf.filled_state(_keys(), tag, torch.float32), strict=True)
    return model.to(dev())


def _bound(g, name):
    return max(3.0 * float(g["floor/" + name]), PARITY)


def test_protocol_vs_reference_golden():
    """Three Adam iterations at B = 4 pairs from a conditioned state: logits and loss of every iteration, every parameter's gradient
    of iteration 0, the BatchNorms' running statistics after every iteration and every parameter after the third, each within
    max(3 x the reference's own fp32-vs-fp64 deviation, 1e-3) relative L2.  The four conv biases in front of a BatchNorm are the
    exception: their gradient is mathematically zero (checked against the layer's weight-gradient norm), so Adam turns rounding noise
    into +-lr steps in either implementation, and their final values are only checked to lie within 3 lr of the initial ones."""
    from optimalstrategiesagainstgenerativeattacks_amd.baseline_training import SiameseTrainer
    g = load_npz("siamese_train.npz")
    model = _model(sf.PROTO_TAG)
    init = {k: v.detach().clone() for k, v in model.named_parameters()}
    tr = SiameseTrainer(model, lr=sf.LR)
    dead_bias = ["embedding_net.encoder.%d.0.bias" % i for i in range(4)]
    errs = {}
    for it in range(sf.PROTO_ITERS):
        x1, x2 = (bf.images("%s%s/it%d" % (sf.PROTO_TAG, nm, it), (sf.PROTO_B, 1, 32, 32), torch.float32).to(dev()) for nm in ("x1", "x2"))
        loss, acc = tr.train_step(x1, x2, sf.PROTO_N_POS)
        errs["it%d/logits" % it] = relerr(tr.last_logits, g["it%d/logits" % it])
        errs["it%d/loss" % it] = relerr(loss, g["it%d/loss" % it])
        if it == 0:
            for k, p in model.named_parameters():
                if k in dead_bias:
                    wnorm = float(np.linalg.norm(g["grad/" + k.replace("bias", "weight")]))
                    e = relerr_floor(p.grad, g["grad/" + k], wnorm)
                    print("grad/%s (zero in exact arithmetic): %.2e of the weight gradient's norm" % (k, e))
                    assert e < PARITY, (k, e)
                else:
                    errs["grad/" + k] = relerr(p.grad, g["grad/" + k])
        for k, v in model.state_dict().items():
            if k.endswith(("running_mean", "running_var")):
                errs["it%d/%s" % (it, k)] = relerr(v, g["it%d/%s" % (it, k)])
            elif k.endswith("num_batches_tracked"):
                assert int(v) == int(g["it%d/%s" % (it, k)]) == 7 + it + 1, (it, k)
    for k, p in model.named_parameters():
        if k in dead_bias:
            moved = float((p.detach() - init[k]).abs().max())
            print("final/%s: moved by at most %.3e (3 lr = %.1e)" % (k, moved, 3 * sf.LR))
            assert moved <= 3 * sf.LR * (1 + 1e-5), (k, moved)
        else:
            errs["final/" + k] = relerr(p, g["final/" + k])
    for name, e in errs.items():
        print("%-50s %.3e  (bound %.3e)" % (name, e, _bound(g, name)))
    for name, e in errs.items():
        assert e < _bound(g, name), (name, e, _bound(g, name))


def _bank(per_class=sf.BANK_PER_CLASS, m=1, n=1, k=1, mirror=True):
    import optimalstrategiesagainstgenerativeattacks_amd as G
    imgs, offs = sf.separable_bank(per_class=per_class)
    return imgs, G.EpisodeBank(torch.from_numpy(imgs).to(dev()), offs, m, n, k, example_cnt_per_class=1, mirror=mirror, seed=5)


def test_loss_curve_vs_reference_golden():
    """40 iterations at B = 16 on the synthetic separable bank, the pairs drawn by PairSampler (the fixture stores what the tool drew):
    the first loss at 1e-3, every 8-iteration window mean of loss and accuracy within max(3 x the reference's own fp32-vs-fp64
    envelope, 1e-3) of the reference's fp64 curve."""
    from optimalstrategiesagainstgenerativeattacks_amd.baseline_training import PairSampler, SiameseTrainer
    g = load_npz("siamese_train.npz")
    imgs, bank = _bank()
    sampler = PairSampler(bank, sf.CURVE_B, sf.CURVE_SEED)
    tr = SiameseTrainer(_model(sf.CURVE_TAG), lr=sf.LR)
    out = []
    for it in range(sf.CURVE_ITERS):
        idx, flip, _ = sampler.draw(it)
        assert np.array_equal(idx, g["curve/idx"][it]) and np.array_equal(flip, g["curve/flip"][it]), it
        x1, x2, n_pos = sampler.batch(it)
        if it == 0:     # the images the reference was trained on
            assert torch.equal(torch.cat([x1, x2]).cpu(), torch.from_numpy(sf.gather_host(imgs, idx.T, flip.T)))
        out.extend(tr.train_step(x1, x2, n_pos))
    curve = torch.stack(out).double().cpu().numpy().reshape(sf.CURVE_ITERS, 2)
    loss, acc = curve[:, 0], curve[:, 1]
    print("loss     ", np.round(loss, 4).tolist())
    print("reference", np.round(g["curve/loss"], 4).tolist())
    print("acc      ", acc.tolist())
    print("reference", g["curve/acc"].tolist())
    assert abs(loss[0] - g["curve/loss"][0]) < PARITY * g["curve/loss"][0]
    for nm, got, ref, env in (("loss", loss, g["curve/loss"], g["curve/env_loss"]), ("acc", acc, g["curve/acc"], g["curve/env_acc"])):
        d = np.abs(sf.window_means(got) - sf.window_means(ref))
        bound = np.maximum(3.0 * env, PARITY)
        print("%s window means: largest deviation %.3e (bound there %.3e)" % (nm, d.max(), bound[d.argmax()]))
        assert (d <= bound).all(), (nm, d.tolist(), bound.tolist())


def test_eval_forward_sees_the_trained_weights():
    """The inference path caches parameters derived from the state dict (BatchNorm folded into the convolutions, fc columns
    permuted); a training step drops that cache: the model's eval-mode logits move, and equal those of a fresh model loaded from the
    trainer's state dict."""
    from optimalstrategiesagainstgenerativeattacks_amd import baselines as bl
    from optimalstrategiesagainstgenerativeattacks_amd.baseline_training import SiameseTrainer
    model = _model(sf.PROTO_TAG).train(mode=False)
    x1, x2 = (bf.images("%s%s/it0" % (sf.PROTO_TAG, nm), (sf.PROTO_B, 1, 32, 32), torch.float32).to(dev()) for nm in ("x1", "x2"))
    with torch.no_grad():
        before = model(x1, x2).clone()
    assert model._derived is not None and model.embedding_net._derived is not None
    tr = SiameseTrainer(model, lr=sf.LR)
    for _ in range(2):
        tr.train_step(x1, x2, sf.PROTO_N_POS)
    assert model._derived is None and model.embedding_net._derived is None and not model.training
    with torch.no_grad():
        after = model(x1, x2)
    assert relerr(after, before) > 1e-3
    enc = bl.ProtonetEmbeddingNet(1, 32)
    fresh = bl.SiameseNet(enc, enc.embedding_dim)
    fresh.load_state_dict(tr.state_dict()["model"], strict=True)
    with torch.no_grad():
        assert torch.equal(fresh.to(dev()).train(mode=False)(x1, x2), after)
    with pytest.raises(RuntimeError, match="inference only"):
        model.train()(x1, x2)


def test_train_resume_and_authentication_table(tmp_path):
    """train_siamese for 6 iterations with a checkpoint every 3; a second run stopped at 3 and resumed reproduces the first one's
    step-6 parameters bit for bit (deterministic mode: no float atomics in the convolutions' weight gradients either);
    get_siamese_authenticator loads the checkpoint and scores as the trained model does; eval_authentication_task writes its six rows
    with the trained baseline."""
    import optimalstrategiesagainstgenerativeattacks_amd as G
    from optimalstrategiesagainstgenerativeattacks_amd import authentication_eval as ae
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    m, n, k, bs = 1, 3, 4, 4
    _, bank = _bank(per_class=10, m=m, n=n, k=k, mirror=False)
    a, b, c0 = (str(tmp_path / d) for d in ("a", "b", "c0"))
    prev = ops.set_deterministic(True)
    try:
        log = G.Logger(log_dir=str(tmp_path / "logs"), img_dir=str(tmp_path / "imgs"))
        tr_a = G.train_siamese(dev(), bank, a, 6, batch_size=16, log_every=2, save_every=3, seed=4, logger=log)
        G.train_siamese(dev(), bank, b, 3, batch_size=16, log_every=2, save_every=3, seed=4)
        G.train_siamese(dev(), bank, b, 6, batch_size=16, log_every=2, save_every=3, seed=4)
        G.train_siamese(dev(), bank, c0, 0, batch_size=16, seed=4)      # the initial state, as a checkpoint
    finally:
        ops.set_deterministic(prev)
    assert [s for s, _ in log.stats["siamese"]["loss"]] == [2, 4, 6] and [s for s, _ in log.stats["siamese"]["acc"]] == [2, 4, 6]
    assert all(np.isfinite(v) and v > 0 for _, v in log.stats["siamese"]["loss"])
    for d in (a, b):
        assert sorted(os.listdir(os.path.join(d, "ckpts"))) == ["model_00000003.pt", "model_00000006.pt"]
        assert json.load(open(os.path.join(d, "args.json")))["img_size"] == 32
    ck_a, ck_b = (torch.load(os.path.join(d, "ckpts", "model_00000006.pt"), map_location="cpu") for d in (a, b))
    assert ck_a["global_step"] == ck_b["global_step"] == 6 and set(ck_a) == {"model", "opt", "global_step"}
    assert [kk for kk in ck_a["model"]] == [e[0] for e in _keys()]
    for kk, v in ck_a["model"].items():
        assert torch.equal(v, ck_b["model"][kk]), kk
    mid = torch.load(os.path.join(b, "ckpts", "model_00000003.pt"), map_location="cpu")["model"]
    assert not torch.equal(mid["fc.weight"], ck_b["model"]["fc.weight"])

    # the checkpoint as the evaluation loads it
    path, args = ae.get_exp_args_from_dir(a, "ckpts")
    assert path.endswith("model_00000006.pt")
    au = ae.get_siamese_authenticator(dev(), path, args)
    au0 = ae.get_siamese_authenticator(dev(), *ae.get_exp_args_from_dir(c0, "ckpts"))
    batch = bank.batch([0, 1, 2, 3])
    test, si = batch["real_sample"][:, :1], batch["si_sample"][:, :1]
    out, pred = au.act(test_sample=test, si_sample=si)
    model = tr_a.model.train(mode=False)
    with torch.no_grad():
        own = model(si[:, 0], test[:, 0]).squeeze()
    assert torch.equal(out, own)
    out0, _ = au0.act(test_sample=test, si_sample=si)
    assert relerr(out, out0) > 1e-3

    # the result table with the trained baseline
    keys = load_keys("32_1_512")
    gim = tmp_path / "gim"
    (gim / "ckpts").mkdir(parents=True)
    torch.save({"authenticator": filled_sd(keys["au"], "e2e/au/", torch.float32), "impersonator": filled_sd(keys["im"], "e2e/im/", torch.float32)},
               str(gim / "ckpts" / "model_00000003.pt"))
    (gim / "args.json").write_text(json.dumps({"target_img_size": 32, "img_channels": 1, "style_dim": 512, "use_img_att": False,
                                               "num_env_noise_layers": 4, "remove_noise_mean": True}))
    bank.root = "synthetic"
    table = str(tmp_path / "out" / "siamese.csv")
    ae.eval_authentication_task(dev(), bank, m, n, k, bs, 0, str(gim), table, baseline_exp_dir=a, baseline_type="siamese")
    with open(table) as f:
        rows = list(csv.DictReader(f))
    assert [(r["au_type"], r["im_type"]) for r in rows] == [(x, i) for x in ("gim", "siamese") for i in ("gim", "replay", "rnd_src")]
    for r in rows:
        for col in ("acc", "acc_on_fake", "acc_on_real", "auc"):
            assert 0.0 <= float(r[col]) <= 1.0, r
