"""Calibrating a trained baseline's decision threshold (authentication_eval.calibrate_baseline) on the MI355X: the tiny shapes of
tests/test_gpu_arcface_training.py / test_gpu_siamese_training.py - the synthetic separable bank, 32 x 32 x 1, 8 classes, batch 8,
two training iterations."""
import csv
import json
import os
import random

import numpy as np
import pytest
import torch

from tests import siamese_fill as sf
from tests.helpers import filled_sd, load_keys

pytestmark = pytest.mark.gpu

M, N, K, BS = 1, 3, 4, 8


def dev():
    return torch.device("cuda:0")


def _bank(seed):
    """A fresh bank: its generators start at `seed`, so two banks of one seed deal the same episodes."""
    import optimalstrategiesagainstgenerativeattacks_amd as G
    imgs, offs = sf.separable_bank(per_class=10)
    bank = G.EpisodeBank(torch.from_numpy(imgs).to(dev()), offs, M, N, K, example_cnt_per_class=4, mirror=False, seed=seed)
    bank.root = "synthetic"
    return bank


def _calibrate_and_check(baseline, exp):
    """calibrate_baseline on a held-out bank; the file it leaves, the authenticator loaded from it, and the stored accuracies
    reproduced by that authenticator's own decisions on the same episodes.  Returns the new args."""
    from optimalstrategiesagainstgenerativeattacks_amd import authentication_eval as ae
    before = json.load(open(os.path.join(exp, "args.json")))
    random.seed(21)
    stats = ae.calibrate_baseline(dev(), baseline, exp, _bank(11), batch_size=BS)
    args = json.load(open(os.path.join(exp, "args.json")))
    assert {kk: v for kk, v in args.items() if kk not in ("th", "th_calibration")} == {kk: v for kk, v in before.items() if kk != "th"}
    cal = args["th_calibration"]
    assert args["th"] == stats["th"] and cal["balanced_acc"] >= 0.5 and cal["acc_on_real"] > 0
    assert cal == dict({kk: stats[kk] for kk in ("auc", "balanced_acc", "acc_on_real", "acc_on_fake", "n_real", "n_fake")},
                       ds_root="synthetic", ckpt="model_00000002.pt")
    assert cal["n_real"] == cal["n_fake"] == 32

    path, loaded = ae.get_exp_args_from_dir(exp, "ckpts")
    au = ae.get_authenticator(dev(), baseline, path, loaded)
    assert au.th == args["th"]
    bank = _bank(11)                       # the same episodes and, with the same seed, the same random sources
    random.seed(21)
    out_r, out_f, pred_r, pred_f = ae.collect_scores(dev(), bank, BS, 0, au, ae.get_impersonator(dev(), "rnd_src", None, bank, None))
    assert ae.roc_statistics(out_r, out_f) == stats == ae.roc_statistics_host(out_r, out_f)
    assert int(pred_r.sum()) == round(stats["acc_on_real"] * 32) and int((pred_f == 0).sum()) == round(stats["acc_on_fake"] * 32)
    _, acc_on_fake, acc_on_real = ae.comp_acc(pred_r, pred_f)
    assert float(acc_on_real) == float(np.float32(stats["acc_on_real"])) and float(acc_on_fake) == float(np.float32(stats["acc_on_fake"]))
    return args


def test_arcface_threshold_is_calibrated(tmp_path):
    import optimalstrategiesagainstgenerativeattacks_amd as G
    from optimalstrategiesagainstgenerativeattacks_amd import authentication_eval as ae
    exp = str(tmp_path / "arcface")
    train = _bank(5)
    G.train_arcface(dev(), train, exp, 2, batch_size=BS, lr=1e-4, seed=4)
    # the defect: the reference's default th = 1.5 against a score -|e1 - e2|^2 <= 0 rejects every real set
    path, args = ae.get_exp_args_from_dir(exp, "ckpts")
    assert args["th"] == 1.5
    batch = train.batch(list(range(8)))
    out, pred = ae.get_arcface_authenticator(dev(), path, args).act(test_sample=batch["real_sample"], si_sample=batch["si_sample"])
    assert float(out.max()) <= 0.0 and int(pred.sum()) == 0
    args = _calibrate_and_check("arcface", exp)
    assert args["th"] <= 0


def test_siamese_threshold_is_calibrated_and_the_table_still_has_six_rows(tmp_path):
    import optimalstrategiesagainstgenerativeattacks_amd as G
    from optimalstrategiesagainstgenerativeattacks_amd import authentication_eval as ae
    exp = str(tmp_path / "siamese")
    G.train_siamese(dev(), _bank(5), exp, 2, batch_size=BS, seed=4)
    path, args = ae.get_exp_args_from_dir(exp, "ckpts")
    assert "th" not in args and ae.get_siamese_authenticator(dev(), path, args).th == 0
    _calibrate_and_check("siamese", exp)

    keys = load_keys("32_1_512")
    gim = tmp_path / "gim"
    (gim / "ckpts").mkdir(parents=True)
    torch.save({"authenticator": filled_sd(keys["au"], "e2e/au/", torch.float32), "impersonator": filled_sd(keys["im"], "e2e/im/", torch.float32)},
               str(gim / "ckpts" / "model_00000003.pt"))
    (gim / "args.json").write_text(json.dumps({"target_img_size": 32, "img_channels": 1, "style_dim": 512, "use_img_att": False,
                                               "num_env_noise_layers": 4, "remove_noise_mean": True}))
    table = str(tmp_path / "out" / "siamese.csv")
    ae.eval_authentication_task(dev(), _bank(7), M, N, K, BS, 0, str(gim), table, baseline_exp_dir=exp, baseline_type="siamese")
    with open(table) as f:
        rows = list(csv.DictReader(f))
    assert [(r["au_type"], r["im_type"]) for r in rows] == [(x, i) for x in ("gim", "siamese") for i in ("gim", "replay", "rnd_src")]
    for r in rows:
        for col in ("acc", "acc_on_fake", "acc_on_real", "auc"):
            assert 0.0 <= float(r[col]) <= 1.0, r
