"""Data-parallel baseline training, two ranks: two child processes on the one card with gloo between them
(tests/baseline_dp_worker.py) run the three-step protocols of tests/test_gpu_siamese_training.py and tests/test_gpu_arcface_training.py
with each rank on its half of the batch, and the parent asserts against the same fixtures (tests/golden/siamese_train.npz,
arcface_train.npz: the REFERENCE's model trained by torch on the whole batch) with the same bounds.  A tree that only sliced the
batches would fail them: per-rank statistics over 4 images are far outside 1e-3 of the whole batch's.  Every test is a single shot."""
import csv
import json
import math
import os
import socket
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from tests import arcface_fill as af
from tests import siamese_fill as sf
from tests.helpers import filled_sd, load_keys, load_npz, relerr, relerr_floor

PARITY = 1e-3       # siamese: the project's parity contract against the reference
BLOCK = 1e-4        # arcface: emb, logits, loss, gradients against the reference
STATS = 3e-5        # arcface: running statistics (one operator)
WORLD = 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def run_ranks(mode, out_dir, limit, env=None):
    """Starts one worker per rank on a fresh loopback port and waits for them.  The first child that exits non-zero ends the run: its
    sibling is killed and nothing further is started.  limit: seconds the whole run may take (sized to the run by the caller)."""
    os.makedirs(out_dir, exist_ok=True)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = str(s.getsockname()[1])
    child_env = dict(os.environ, **(env or {}))
    logs = [open(os.path.join(out_dir, "rank%d.log" % r), "w+") for r in range(WORLD)]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "baseline_dp_worker.py"), mode, str(r), str(WORLD), port, out_dir],
                              cwd=ROOT, env=child_env, stdout=logs[r], stderr=subprocess.STDOUT) for r in range(WORLD)]
    deadline = time.monotonic() + limit
    failed = None
    try:
        running = list(range(WORLD))
        while running and failed is None:
            for r in list(running):
                try:
                    rc = procs[r].wait(timeout=0.1)
                except subprocess.TimeoutExpired:
                    continue
                running.remove(r)
                if rc != 0:
                    failed = "rank %d exited with %d" % (r, rc)
            if running and failed is None and time.monotonic() > deadline:
                failed = "ranks %s still running after %d s" % (running, limit)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
            p.wait()
    tails = []
    for r, f in enumerate(logs):
        f.seek(0)
        tails.append("---- rank %d ----\n%s" % (r, f.read()[-3000:]))
        f.close()
    assert failed is None, "%s\n%s" % (failed, "\n".join(tails))
    return [torch.load(os.path.join(out_dir, "result%d.pt" % r), map_location="cpu", weights_only=False) for r in range(WORLD)]


def assert_replicas_equal(out_dir, ref_keys=None):
    a, b = (torch.load(os.path.join(out_dir, "state%d.pt" % r), map_location="cpu") for r in range(WORLD))
    assert list(a) == list(b) and (ref_keys is None or list(a) == ref_keys)
    for k in a:
        assert torch.equal(a[k], b[k]), "the ranks' %s differ by up to %.3e" % (k, float((a[k].double() - b[k].double()).abs().max()))
    return a


def test_siamese_protocol_two_ranks_vs_reference_golden(tmp_path):
    """test_protocol_vs_reference_golden of tests/test_gpu_siamese_training.py on two ranks: B = 4 pairs, rank 0 has the two positive
    pairs and rank 1 none, each encoder pass is 4 images.  Logits (global row order) and the rank-mean loss of every iteration,
    every parameter's iteration-0 gradient (the all-reduced bucket / world), the running statistics after every iteration and the
    final parameters within max(3 x floor, 1e-3), the dead conv biases by their own rules; the ranks' final state dicts are equal
    bit for bit, though they never exchanged a parameter or a buffer."""
    g = load_npz("siamese_train.npz")
    res = run_ranks("siamese", str(tmp_path), 150)[0]
    assert res["n_pos"] == [2, 0]
    bound = lambda name: max(3.0 * float(g["floor/" + name]), PARITY)
    dead_bias = ["embedding_net.encoder.%d.0.bias" % i for i in range(4)]
    names = list(res["init"])
    errs = {}
    for it in range(sf.PROTO_ITERS):
        errs["it%d/logits" % it] = relerr(res["it%d/logits" % it], g["it%d/logits" % it])
        errs["it%d/loss" % it] = relerr(res["it%d/loss" % it], g["it%d/loss" % it])
        for k in [k[len("it%d/" % it):] for k in res if k.startswith("it%d/" % it)]:
            if k.endswith(("running_mean", "running_var")):
                errs["it%d/%s" % (it, k)] = relerr(res["it%d/%s" % (it, k)], g["it%d/%s" % (it, k)])
            elif k.endswith("num_batches_tracked"):
                assert int(res["it%d/%s" % (it, k)]) == int(g["it%d/%s" % (it, k)]) == 7 + it + 1, (it, k)
    assert sum(k.endswith("running_var") for k in errs) == 4 * sf.PROTO_ITERS
    for k in names:
        if k in dead_bias:
            wnorm = float(np.linalg.norm(g["grad/" + k.replace("bias", "weight")]))
            e = relerr_floor(res["grad/" + k], g["grad/" + k], wnorm)
            print("grad/%s (zero in exact arithmetic, over both ranks): %.2e of the weight gradient's norm" % (k, e))
            assert e < PARITY, (k, e)
            moved = float((res["final/" + k] - res["init"][k]).abs().max())
            print("final/%s: moved by at most %.3e (3 lr = %.1e)" % (k, moved, 3 * sf.LR))
            assert moved <= 3 * sf.LR * (1 + 1e-5), (k, moved)
        else:
            errs["grad/" + k] = relerr(res["grad/" + k], g["grad/" + k])
            errs["final/" + k] = relerr(res["final/" + k], g["final/" + k])
    for name, e in errs.items():
        print("%-50s %.3e  (bound %.3e)" % (name, e, bound(name)))
    for name, e in errs.items():
        assert e < bound(name), (name, e, bound(name))
    assert_replicas_equal(str(tmp_path))


def test_arcface_protocol_two_ranks_vs_reference_golden(tmp_path):
    """test_protocol_vs_reference_golden of tests/test_gpu_arcface_training.py on two ranks: B = 8, 4 images per rank, lr = 1e-5, three
    iterations; the last stage's maps are 2 x 2 and the BatchNorm1d sees 4 rows per rank.  The assertions and bounds are that test's
    (BLOCK, STATS, the small-tensor rule, the first-update rule), gradients again as the all-reduced bucket / world; the ranks' final
    state dicts are equal bit for bit.

    The workers run in deterministic mode (GIM_DETERMINISTIC=1).  DESIGN.md section 10 records an open, machine-dependent deviation
    of the default mode's split-K input gradients on the 4 x 4 maps in exactly this protocol; deterministic mode has passed
    wherever it was tried.  This test is about the data-parallel path, not about that observation."""
    gold = load_npz("arcface_train.npz")
    res = run_ranks("arcface", str(tmp_path), 280, {"GIM_DETERMINISTIC": "1"})[0]
    names = res["names"]
    assert names == list(gold["grad_names"]) == [k for k, _ in af.parameter_entries()]
    small = set(gold["small"].tolist())
    g_ref, d_ref = af.unpack(gold["grad"]), af.unpack(gold["delta"], af.delta_index)
    norms, floors = dict(zip(names, gold["gradnorm"])), dict(zip(names, gold["floor_grad"]))
    numel = dict(af.parameter_entries())
    largest = max(norms.values())
    errs, bounds = {}, {}
    for it in range(af.PROTO_ITERS):
        for nm in ("emb", "logits", "loss"):
            key = "it%d/%s" % (it, nm)
            errs[key], bounds[key] = relerr(res[key], gold[key]), max(3.0 * float(gold["floor/" + key]), BLOCK)
        for bn in af.RUNNING:
            for leaf in ("running_mean", "running_var"):
                key = "it%d/run/%s.%s" % (it, bn, leaf)
                errs[key], bounds[key] = relerr(res[key], gold[key]), max(3.0 * float(gold["floor/" + key]), STATS)
            assert int(res["it%d/run/%s.num_batches_tracked" % (it, bn)]) == 7 + it + 1
    worst_update, masked, total = 0.0, 0, 0
    for k in names:
        if k in small:
            e = res["gradnorm/" + k] / largest
            print("grad/%s (small): %.2e of the largest gradient norm" % (k, e))
            assert e <= 1e-5, (k, e)
            continue
        errs["grad/" + k] = relerr(res["grad/" + k], g_ref[k])
        bounds["grad/" + k] = max(3.0 * float(floors[k]), BLOCK)
        gr = torch.from_numpy(g_ref[k][::2]).double()
        keep = gr.abs() >= af.MASK_REL * float(norms[k]) / math.sqrt(numel[k])
        d = (res["delta/" + k] - torch.from_numpy(d_ref[k]).double()).abs()[keep]
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
    assert_replicas_equal(str(tmp_path), [e[0] for e in af.keys()])


def test_train_loop_two_ranks_writes_once_resumes_and_evaluates(tmp_path):
    """train_siamese on two ranks to iteration 4 and, in a second call, on to 6 (a checkpoint every 2, a log point every 2): one
    checkpoint set and one args.json, written by rank 0; only rank 0 logged, the second call from the resumed iteration on; the ranks
    end with equal state dicts, which are the last checkpoint's; and the checkpoint loads into the authentication evaluation."""
    import optimalstrategiesagainstgenerativeattacks_amd as G
    from optimalstrategiesagainstgenerativeattacks_amd import authentication_eval as ae
    res = run_ranks("loop", str(tmp_path), 150, {"GIM_DETERMINISTIC": "1"})
    exp = str(tmp_path / "exp")
    assert sorted(os.listdir(exp)) == ["args.json", "ckpts"]
    assert sorted(os.listdir(os.path.join(exp, "ckpts"))) == ["model_%08d.pt" % s for s in (2, 4, 6)]       # no rank-1 copies, no temporaries
    args = json.load(open(os.path.join(exp, "args.json")))
    assert args["batch_size"] == 8 and args["n_iters"] == 6 and args["baseline_type"] == "siamese"
    first, second = res[0]["logs"]
    assert [s for s, _ in first["loss"]] == [2, 4] and [s for s, _ in second["loss"]] == [6] and [s for s, _ in second["acc"]] == [6]
    assert all(np.isfinite(v) and v > 0 for _, v in first["loss"] + second["loss"]) and all(0.0 <= v <= 1.0 for _, v in first["acc"] + second["acc"])
    assert res[1]["logs"] == [{}, {}]
    state = assert_replicas_equal(str(tmp_path))
    ck = torch.load(os.path.join(exp, "ckpts", "model_00000006.pt"), map_location="cpu")
    assert ck["global_step"] == 6 and set(ck) == {"model", "opt", "global_step"}
    for k, v in ck["model"].items():
        assert torch.equal(v, state[k]), k
    mid = torch.load(os.path.join(exp, "ckpts", "model_00000004.pt"), map_location="cpu")["model"]
    assert not torch.equal(mid["fc.weight"], ck["model"]["fc.weight"])

    # the checkpoint as the evaluation loads it (tests/test_gpu_siamese_training.py's round trip)
    m, n, k, bs = 1, 3, 4, 4
    imgs, offs = sf.separable_bank(per_class=10)
    bank = G.EpisodeBank(torch.from_numpy(imgs).to(dev()), offs, m, n, k, example_cnt_per_class=1, mirror=False, seed=5)
    path, eargs = ae.get_exp_args_from_dir(exp, "ckpts")
    assert path.endswith("model_00000006.pt")
    au = ae.get_siamese_authenticator(dev(), path, eargs)
    batch = bank.batch([0, 1, 2, 3])
    out, _ = au.act(test_sample=batch["real_sample"][:, :1], si_sample=batch["si_sample"][:, :1])
    assert torch.isfinite(out).all()
    keys = load_keys("32_1_512")
    gim = tmp_path / "gim"
    (gim / "ckpts").mkdir(parents=True)
    torch.save({"authenticator": filled_sd(keys["au"], "e2e/au/", torch.float32), "impersonator": filled_sd(keys["im"], "e2e/im/", torch.float32)},
               str(gim / "ckpts" / "model_00000003.pt"))
    (gim / "args.json").write_text(json.dumps({"target_img_size": 32, "img_channels": 1, "style_dim": 512, "use_img_att": False,
                                               "num_env_noise_layers": 4, "remove_noise_mean": True}))
    bank.root = "synthetic"
    table = str(tmp_path / "out" / "siamese.csv")
    ae.eval_authentication_task(dev(), bank, m, n, k, bs, 0, str(gim), table, baseline_exp_dir=exp, baseline_type="siamese")
    with open(table) as f:
        rows = list(csv.DictReader(f))
    assert [(r["au_type"], r["im_type"]) for r in rows] == [(x, i) for x in ("gim", "siamese") for i in ("gim", "replay", "rnd_src")]
    for r in rows:
        for col in ("acc", "acc_on_fake", "acc_on_real", "auc"):
            assert 0.0 <= float(r[col]) <= 1.0, r
