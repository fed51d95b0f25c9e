"""The baseline authenticators' inference path on the GPU: the strided convolution entry and the pointwise kernels against
fp64 torch on the CPU, blocks and whole nets against what the REFERENCE's modules gave (tests/golden/baselines.npz, written by
tools/make_baseline_golden.py; weights and images regenerated from names by tests/baseline_fill.py), the result table end to end.
Every test is a single shot."""
import csv
import json
import os
import random

import pytest
import torch
import torch.nn.functional as F

from tests import baseline_fill as bf
from tests.helpers import GOLDEN, filled_sd, load_keys, load_npz, relerr

TOL = 3e-5          # relative L2 over the whole tensor, fp32 kernels against fp64 (tests/test_gpu_tuned_rows.py, tests/test_gpu_ops.py)
TOL_MAX = 2e-4      # largest single-element error relative to the largest reference element
PARITY = 1e-3       # the project's parity contract against the reference (test_eval_mode_forward_vs_oracle)
POINTWISE = 1e-6    # a few fp32 roundings (eps = 6e-8 each)


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _fixture():
    with open(os.path.join(GOLDEN, "baseline_keys.json")) as f:
        return json.load(f)


def _build(cfg):
    from optimalstrategiesagainstgenerativeattacks_amd import baselines as bl
    c = bf.CONFIGS[cfg]
    if c["kind"] == "siamese":
        enc = bl.ProtonetEmbeddingNet(c["img_channels"], c["img_size"])
        return bl.SiameseNet(enc, enc.embedding_dim)
    return bl.ArcFace(bl.Backbone(c["num_layers"], 0.6, 'ir_se', c["img_size"], c["img_channels"]), 512, c["n_classes"])


def _filled(cfg, tag=None):
    model = _build(cfg)
    model.load_state_dict(bf.filled_state(_fixture()["keys"][cfg], tag or "bl/%s/" % cfg, torch.float32), strict=True)
    return model.to(dev()).train(mode=False)


# ------------------------------------------------------------------------------------------------------
# 5. gim_conv2d_infer, every distinct launch shape of the two networks
# ------------------------------------------------------------------------------------------------------
def conv_launch_shapes():
    """Distinct (H, Cin, Cout, KH, stride) of every convolution / linear launch of ArcFace-50 at 64x64x3 and 32x32x1 and of the
    siamese net at 32x32x1 (H = W = 1: the SE and output linears)."""
    from optimalstrategiesagainstgenerativeattacks_amd.baselines import unit_plan
    shapes = set()
    for S, C in ((64, 3), (32, 1)):
        shapes.add((S, C, 64, 3, 1))
        H = S
        for cin, depth, stride in unit_plan(50):
            shapes.add((H, cin, depth, 3, 1))
            shapes.add((H, depth, depth, 3, stride))
            if cin != depth:
                shapes.add((H, cin, depth, 1, stride))
            shapes.add((1, depth, depth // 16, 1, 1))
            shapes.add((1, depth // 16, depth, 1, 1))
            H //= stride
        shapes.add((1, 512 * H * H, 512, 1, 1))
    H, cin = 32, 1
    for _ in range(4):
        shapes.add((H, cin, 64, 3, 1))
        H, cin = H // 2, 64
    shapes.add((1, 64 * H * H, 1, 1, 1))
    return sorted(shapes)


SHAPES = conv_launch_shapes()
EXTRA = [(64, 64, 64, 3, 2), (16, 128, 256, 1, 2), (32, 1, 64, 3, 1)]      # also at N = 1 and N = 5, every bias / slope combination
CASES = [(6, s, True, True) for s in SHAPES] + [(6, s, False, False) for s in SHAPES]
CASES += [(N, s, hb, hs) for s in EXTRA for N in (1, 5) for hb in (False, True) for hs in (False, True)]


def _close(got, ref, what):
    ref = ref.to(got.device)
    err = float((got.double() - ref).norm() / ref.norm())
    emax = float((got.double() - ref).abs().max() / ref.abs().max())
    print("%s: relative L2 %.3e, max element %.3e" % (what, err, emax))
    assert err < TOL and emax < TOL_MAX, "%s: relative L2 %.2e (max element %.2e)" % (what, err, emax)


def test_conv_shape_list_covers_both_networks():
    assert all(s in SHAPES for s in EXTRA)
    assert (64, 3, 64, 3, 1) in SHAPES and (4, 512, 512, 3, 1) in SHAPES and (8, 256, 512, 1, 2) in SHAPES
    assert (1, 64, 4, 1, 1) in SHAPES and (1, 32, 512, 1, 1) in SHAPES and (1, 8192, 512, 1, 1) in SHAPES and (1, 256, 1, 1, 1) in SHAPES


@pytest.mark.gpu
@pytest.mark.parametrize("N,shape,has_bias,has_slope", CASES,
                         ids=["N%d-%s-b%d-s%d" % (N, "x".join(map(str, s)), hb, hs) for N, s, hb, hs in CASES])
def test_conv2d_infer_elementwise_vs_fp64_conv2d(N, shape, has_bias, has_slope):
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    H, Cin, Cout, K, stride = shape
    g = torch.Generator().manual_seed(1000 * H + 7 * Cin + Cout + K + stride + N)
    x = torch.randn(N, Cin, H, H, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, Cin, K, K, generator=g, dtype=torch.float64) / (Cin * K * K) ** 0.5
    b = torch.randn(Cout, generator=g, dtype=torch.float64) if has_bias else None
    a = (torch.rand(Cout, generator=g, dtype=torch.float64) * 0.5 - 0.1) if has_slope else None
    x, w = x.float().double(), w.float().double()                      # the values the kernel sees
    b = None if b is None else b.float().double()
    a = None if a is None else a.float().double()
    ref = F.conv2d(x, w, b, stride, (K - 1) // 2)
    if a is not None:
        ref = torch.where(ref >= 0, ref, ref * a.view(1, -1, 1, 1))
    with torch.no_grad():
        got = ops.conv2d_infer(x.permute(0, 2, 3, 1).contiguous().float().to(dev()), w.permute(0, 2, 3, 1).contiguous().float().to(dev()),
                               None if b is None else b.float().to(dev()), None if a is None else a.float().to(dev()), stride)
    assert tuple(got.shape) == (N, H // stride, H // stride, Cout)
    _close(got.cpu(), ref.permute(0, 2, 3, 1), "conv2d_infer %s N=%d" % (shape, N))


@pytest.mark.gpu
def test_conv2d_infer_refuses_grad_and_cpu():
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    x = torch.zeros(1, 4, 4, 16, device=dev(), requires_grad=True)
    w = torch.zeros(16, 3, 3, 16, device=dev())
    with pytest.raises(RuntimeError, match="inference operator"):
        ops.conv2d_infer(x, w)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.conv2d_infer(torch.zeros(1, 4, 4, 16), w)
    with torch.no_grad(), pytest.raises(RuntimeError):
        ops.conv2d_infer(x, torch.zeros(16, 5, 5, 16, device=dev()))       # KH in {1, 3}


# ------------------------------------------------------------------------------------------------------
# 6. pointwise kernels
# ------------------------------------------------------------------------------------------------------
def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("N,C", [(3, 64), (5, 512)])
def test_maxpool2_is_exact(N, C):
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    x = _rand(N, 8, 8, C, seed=N + C)
    with torch.no_grad():
        got, got_relu = ops.maxpool2(x.to(dev())), ops.maxpool2(x.to(dev()), relu=True)
    ref = F.max_pool2d(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    assert torch.equal(got.cpu(), ref)
    assert torch.equal(got_relu.cpu(), F.max_pool2d(torch.relu(x).permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1))


@pytest.mark.gpu
@pytest.mark.parametrize("N,C", [(3, 64), (5, 512)])
def test_channel_affine_vs_fp64(N, C):
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    x, s, t = _rand(N, 4, 4, C, seed=1), _rand(C, seed=2), _rand(C, seed=3)
    with torch.no_grad():
        got = ops.channel_affine(x.to(dev()), s.to(dev()), t.to(dev()))
    err = relerr(got, x.double() * s.double() + t.double())
    print("channel_affine relerr %.3e" % err)
    assert err < POINTWISE


@pytest.mark.gpu
@pytest.mark.parametrize("N,C,ss,with_bn", [(3, 64, 1, False), (3, 64, 2, True), (5, 512, 2, False), (5, 512, 1, True)])
def test_se_tail_vs_fp64(N, C, ss, with_bn):
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    Ho = 4
    res, gate, sc = _rand(N, Ho, Ho, C, seed=4), 2 * _rand(N, C, seed=5), _rand(N, Ho * ss, Ho * ss, C, seed=6)
    s, t = _rand(C, seed=7), _rand(C, seed=8)
    ref = res.double() * torch.sigmoid(gate.double()).view(N, 1, 1, C) + sc.double()[:, ::ss, ::ss]
    with torch.no_grad():
        if with_bn:
            out, out_bn = ops.se_tail(res.to(dev()), gate.to(dev()), sc.to(dev()), ss, s.to(dev()), t.to(dev()))
        else:
            out, out_bn = ops.se_tail(res.to(dev()), gate.to(dev()), sc.to(dev()), ss), None
    err = relerr(out, ref)
    print("se_tail relerr %.3e" % err)
    assert err < POINTWISE
    if with_bn:
        err = relerr(out_bn, ref * s.double() + t.double())
        print("se_tail second output relerr %.3e" % err)
        assert err < POINTWISE


@pytest.mark.gpu
@pytest.mark.parametrize("B,D", [(3, 64), (5, 512)])
def test_pair_score_l2norm_absdiff_vs_fp64(B, D):
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    a, b = _rand(B, D, seed=9), _rand(B, D, seed=10)
    b[0] = a[0] * 1.5 + 1e-3 * b[0]                                  # a near-identical direction: the score is close to 0
    ad, bd = a.double(), b.double()
    na, nb = ad / ad.norm(dim=1, keepdim=True), bd / bd.norm(dim=1, keepdim=True)
    with torch.no_grad():
        score, nrm, diff = ops.pair_score(a.to(dev()), b.to(dev())), ops.l2norm_rows(a.to(dev())), ops.absdiff(a.to(dev()), b.to(dev()))
    errs = (relerr(score, -((na - nb) ** 2).sum(1)), relerr(nrm, na), relerr(diff, (ad - bd).abs()))
    print("pair_score %.3e, l2norm_rows %.3e, absdiff %.3e" % errs)
    assert max(errs) < POINTWISE


# ------------------------------------------------------------------------------------------------------
# 7. blocks and nets against the reference's outputs
# ------------------------------------------------------------------------------------------------------
def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous().float().to(dev())


@pytest.mark.gpu
def test_siamese_conv_block_vs_reference():
    """(i) one _conv_block (encoder.1 of the filled siamese net) on a 16x16 map, 3 images."""
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    model = _filled("siamese_32_1")
    w, b = model.embedding_net.derived()["blocks"][1]
    with torch.no_grad():
        got = ops.maxpool2(ops.conv2d_infer(_nhwc(bf.images("bl/block_conv/x", (3, 64, 16, 16))), w, b), relu=True)
    err = relerr(got.permute(0, 3, 1, 2), load_npz("baselines.npz")["block_conv"])
    print("conv block relerr %.3e" % err)
    assert err < PARITY


@pytest.mark.gpu
@pytest.mark.parametrize("cin,depth,stride", [(64, 64, 2), (64, 128, 2), (128, 128, 1)])
def test_ir_se_unit_vs_reference(cin, depth, stride):
    """(ii) bottleneck_IR_SE on 16x16 maps, 3 images: the unit's own leading BatchNorm by channel_affine, then run_unit; the
    second output of its se_tail (the NEXT unit's BatchNorm) is checked against the first."""
    from optimalstrategiesagainstgenerativeattacks_amd import baselines as bl, ops
    fx = _fixture()
    name = "unit_%d_%d_%d" % (cin, depth, stride)
    idx = fx["meta"]["unit_body_index"][name]
    arc = _build("arcface50_64_3")
    unit = arc.emb_model.body[idx]
    assert (unit.cin, unit.depth, unit.stride) == (cin, depth, stride)
    pre = "emb_model.body.%d." % idx
    sd = bf.filled_state([e for e in fx["keys"]["arcface50_64_3"] if e[0].startswith(pre)], "bl/arcface50_64_3/", prefix=pre)
    d = bl._to_device(bl.derive_unit({k: v.float().double() for k, v in sd.items() if v.is_floating_point()}, "", unit), dev())
    x = _nhwc(bf.images("bl/%s/x" % name, (3, cin, 16, 16)))
    s, t = torch.linspace(0.5, 1.5, depth).to(dev()), torch.linspace(-1, 1, depth).to(dev())
    with torch.no_grad():
        xb = ops.channel_affine(x, *d["bn_in"])
        out = bl.run_unit(x, xb, d, stride)
        out2, out_bn = bl.run_unit(x, xb, d, stride, (s, t))
    err = relerr(out.permute(0, 3, 1, 2), load_npz("baselines.npz")[name])
    print("%s relerr %.3e" % (name, err))
    assert err < PARITY
    assert torch.equal(out, out2) and relerr(out_bn, out.double() * s.double() + t.double()) < POINTWISE


def _decisions_equal(got, ref, th, what):
    got, ref = torch.as_tensor(got).cpu().double().view(-1), torch.as_tensor(ref).double().view(-1)
    assert got.numel() == ref.numel()
    assert torch.equal(got >= th, ref >= th), "%s: decisions differ from the reference's: %s vs %s (th %g)" % (what, got.tolist(), ref.tolist(), th)


@pytest.mark.gpu
def test_siamese_net_vs_reference():
    """(iii) embeddings of the test set and the authenticator's logits, B = 4, n = 5, k = 3 at 32x32x1."""
    from optimalstrategiesagainstgenerativeattacks_amd import authentication_eval as ae
    g, fx = load_npz("baselines.npz"), _fixture()["meta"]["fp32_vs_fp64"]
    model = _filled("siamese_32_1")
    tag = "bl/siamese_32_1/"
    test, si = bf.images(tag + "test", (4, 5, 1, 32, 32)).float().to(dev()), bf.images(tag + "si", (4, 3, 1, 32, 32)).float().to(dev())
    emb = model.embedding_net.to_reference_order(model.encode(test.view(20, 1, 32, 32)))
    logits = ae.get_siamese_au_function(model)(test_sample=test, si_sample=si)
    e_emb, e_log = relerr(emb, g["siamese_emb"]), relerr(logits, g["siamese_logits"])
    print("siamese embedding relerr %.3e (reference fp32 vs fp64: %.3e, fixture check %.3e)"
          % (e_emb, fx["siamese_emb"], relerr(g["siamese_emb_f32"], g["siamese_emb"])))
    print("siamese logits    relerr %.3e (reference fp32 vs fp64: %.3e)" % (e_log, fx["siamese_logits"]))
    assert e_emb < PARITY and e_log < PARITY
    _decisions_equal(logits, g["siamese_logits"], 0.0, "siamese")
    _decisions_equal(g["siamese_logits_f32"], g["siamese_logits"], 0.0, "siamese (reference fp32)")


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ["arcface50_64_3", "arcface50_32_1"])
def test_arcface_vs_reference(cfg):
    """(iv) ArcFace-50 embeddings of 4 images and the authenticator's scores for B = 4, n = 5, k = 5."""
    from optimalstrategiesagainstgenerativeattacks_amd import authentication_eval as ae
    g, meta = load_npz("baselines.npz"), _fixture()["meta"]
    c = bf.CONFIGS[cfg]
    S, C = c["img_size"], c["img_channels"]
    arc = _filled(cfg)
    arc.th = meta[cfg + "_th"]
    tag = "bl/%s/" % cfg
    emb = arc.emb_model(bf.images(tag + "x", (4, C, S, S)).float().to(dev()))
    test, si = bf.images(tag + "test", (4, 5, C, S, S)).float().to(dev()), bf.images(tag + "si", (4, 5, C, S, S)).float().to(dev())
    score = ae.get_arcface_au_function(arc)(test_sample=test, si_sample=si)
    e_emb, e_sc = relerr(emb, g[cfg + "_emb"]), relerr(score, g[cfg + "_score"])
    print("%s embedding relerr %.3e (reference fp32 vs fp64: %.3e)" % (cfg, e_emb, meta["fp32_vs_fp64"][cfg + "_emb"]))
    print("%s scores    relerr %.3e (reference fp32 vs fp64: %.3e)" % (cfg, e_sc, meta["fp32_vs_fp64"][cfg + "_score"]))
    assert e_emb < PARITY and e_sc < PARITY
    _decisions_equal(score, g[cfg + "_score"], arc.th, cfg)
    _decisions_equal(g[cfg + "_score_f32"], g[cfg + "_score"], arc.th, cfg + " (reference fp32)")
    _, pred = ae.Authenticator(ae.get_arcface_au_function(arc), th=arc.th).act(test_sample=test, si_sample=si)
    assert pred.cpu().tolist() == (torch.as_tensor(g[cfg + "_score"]) >= arc.th).long().tolist()
    assert 0 < int(pred.sum()) < 4                                    # the threshold separates the fixture batch


# ------------------------------------------------------------------------------------------------------
# 8. the result table end to end
# ------------------------------------------------------------------------------------------------------
class _RecordingBank:
    """The bank, remembering the batches of every pass and the state of `random` when the pass began."""

    def __init__(self, bank):
        self.bank, self.passes, self.root = bank, [], "synthetic"

    def __len__(self):
        return len(self.bank)

    def __getitem__(self, i):
        return self.bank[i]

    def num_batches(self, batch_size, drop_last=True):
        return self.bank.num_batches(batch_size, drop_last)

    def gpu_batches(self, *a, **kw):
        rec = {"random": random.getstate(), "batches": []}
        self.passes.append(rec)
        for b in self.bank.gpu_batches(*a, **kw):
            rec["batches"].append(b)
            yield b


def _write_experiments(tmp_path):
    import optimalstrategiesagainstgenerativeattacks_amd as G
    fx = _fixture()["keys"]
    keys = load_keys("32_1_512")
    gim = tmp_path / "gim"
    (gim / "ckpts").mkdir(parents=True)
    torch.save({"authenticator": filled_sd(keys["au"], "e2e/au/", torch.float32), "impersonator": filled_sd(keys["im"], "e2e/im/", torch.float32)},
               str(gim / "ckpts" / "model_00000003.pt"))
    (gim / "args.json").write_text(json.dumps({"target_img_size": 32, "img_channels": 1, "style_dim": 512, "use_img_att": False,
                                               "num_env_noise_layers": 4, "remove_noise_mean": True}))
    sia = tmp_path / "siamese"
    (sia / "ckpts").mkdir(parents=True)
    torch.save({"model": bf.filled_state(fx["siamese_32_1"], "e2e/siamese/", torch.float32)}, str(sia / "ckpts" / "model_00000001.pt"))
    (sia / "args.json").write_text(json.dumps({"img_size": 32, "img_channels": 1}))
    arc = tmp_path / "arcface"
    (arc / "ckpts").mkdir(parents=True)
    torch.save({"arcface": bf.filled_state(fx["arcface50_32_1"], "e2e/arcface/", torch.float32)}, str(arc / "ckpts" / "model_00000007.pt"))
    (arc / "args.json").write_text(json.dumps({"img_size": 32, "img_channels": 1, "num_layers": 50, "dropout": 0.6, "emb_dim": 512, "th": -0.4}))
    # the GIM state dicts load into the engine's models
    G.get_au(32, 1, 512).load_state_dict(torch.load(str(gim / "ckpts" / "model_00000003.pt"))["authenticator"])
    return str(gim), str(sia), str(arc)


@pytest.mark.gpu
def test_result_table_end_to_end(tmp_path):
    import optimalstrategiesagainstgenerativeattacks_amd as G
    from optimalstrategiesagainstgenerativeattacks_amd import authentication_eval as ae
    gim, sia, arc = _write_experiments(tmp_path)
    m, n, k, bs = 1, 3, 4, 4
    imgs, offs = G.synthetic_bank(8, 10, 32, 1, dev(), seed=2)
    tables = {}
    for baseline, exp in (("siamese", sia), ("arcface", arc)):
        ds = _RecordingBank(G.EpisodeBank(imgs, offs, m, n, k, example_cnt_per_class=1, mirror=False, seed=5))
        random.seed(17)
        torch.manual_seed(3)
        path = str(tmp_path / "out" / (baseline + ".csv"))
        ae.eval_authentication_task(dev(), ds, m, n, k, bs, 0, gim, path, baseline_exp_dir=exp, baseline_type=baseline)
        with open(path) as f:
            rows = list(csv.DictReader(f))
        assert [(r["au_type"], r["im_type"]) for r in rows] == [(a, i) for a in ("gim", baseline) for i in ("gim", "replay", "rnd_src")]
        for r in rows:
            assert r["ds_root"] == "synthetic" and r["gim_exp_dir"] == gim and (r["m"], r["n"], r["k"]) == ("1", "3", "4")
            for col in ("acc", "acc_on_fake", "acc_on_real", "auc"):
                assert 0.0 <= float(r[col]) <= 1.0, (baseline, r)
        assert len(ds.passes) == 6 and all(len(p["batches"]) == 2 for p in ds.passes)
        tables[baseline] = (rows, ds)
    # siamese vs. replay by hand: the same batches, the same state of `random`, through SiameseNet.encode / classify
    rows, ds = tables["siamese"]
    model = _build("siamese_32_1")
    model.load_state_dict(torch.load(os.path.join(sia, "ckpts", "model_00000001.pt"))["model"], strict=True)
    model = model.to(dev()).train(mode=False)
    rec = ds.passes[4]
    random.setstate(rec["random"])
    o_r, o_f = [], []

    def logits(test, si_):
        B = test.shape[0]
        te = model.encode(test.reshape(-1, 1, 32, 32)).view(B, test.shape[1], -1).mean(1)
        se = model.encode(si_.reshape(-1, 1, 32, 32)).view(B, si_.shape[1], -1).mean(1)
        return model.classify(se, te).view(-1)
    for b in rec["batches"]:
        o_r.append(logits(b["real_sample"], b["si_sample"]))
        o_f.append(logits(ae.replay_impersonator(b["leaked_sample"], n), b["si_sample"]))
    o_r, o_f = torch.cat(o_r), torch.cat(o_f)
    acc = 0.5 * ((o_r >= 0).float().mean() + (o_f < 0).float().mean())
    assert rows[4]["au_type"] == "siamese" and rows[4]["im_type"] == "replay"
    assert abs(float(rows[4]["acc"]) - float(acc)) < 1e-6


# ------------------------------------------------------------------------------------------------------
# 9. derived parameters follow the state; the path is deterministic
# ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ["siamese_32_1", "arcface50_32_1"])
def test_reload_refreshes_derived_parameters_and_forward_is_deterministic(cfg):
    entries = _fixture()["keys"][cfg]
    x = bf.images("reload/x", (5, 1, 32, 32)).float().to(dev())
    model = _filled(cfg, "reload/A/")
    net = model.embedding_net if cfg.startswith("siamese") else model.emb_model
    ya, ya2 = net(x), net(x)
    assert torch.equal(ya, ya2)                                       # no atomics on this path
    model.load_state_dict({k: v.to(dev()) for k, v in bf.filled_state(entries, "reload/B/", torch.float32).items()}, strict=True)
    yb = net(x)
    fresh = _filled(cfg, "reload/B/")
    yb_fresh = (fresh.embedding_net if cfg.startswith("siamese") else fresh.emb_model)(x)
    assert torch.equal(yb, yb_fresh) and not torch.equal(ya, yb)
    assert relerr(ya, yb) > 1e-2
