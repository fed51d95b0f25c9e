"""Inference rate of the baseline authenticators (baselines.py): ArcFace-50 at 64x64x3 and the siamese net at 32x32x1, filled
weights, 128 and 512 images per forward.  Prints ONE JSON line: per case images/s, ms per forward (device events around all timed
forwards), and the convolution FLOPs the forward executes (counted from the launch shapes by ops.count_flops) per second over
the fp32 MFMA peak.  That last figure is a WHOLE-FORWARD rate - pointwise passes and launch gaps included - not a kernel's share
of the peak; per-kernel times come from a rocprofv3 --kernel-trace --stats run of this same command.

--layers adds, per distinct convolution launch shape of each case, the time of that launch alone (device events around 20
back-to-back launches on random operands) and its executed TFLOP/s - the figure to hold against the training forward's
same-shaped launches in profiles/*_conv_shapes_*.txt.

    python tools/baseline_infer_bench.py [--steps 50] [--warmup 10] [--layers]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from optimalstrategiesagainstgenerativeattacks_amd import baselines as bl, ops  # noqa: E402
from tests import baseline_fill as bf  # noqa: E402

PEAK_FP32_MFMA = 157.3e12


def build(cfg, dev):
    c = bf.CONFIGS[cfg]
    with open(os.path.join(ROOT, "tests", "golden", "baseline_keys.json")) as f:
        entries = json.load(f)["keys"][cfg]
    if c["kind"] == "siamese":
        enc = bl.ProtonetEmbeddingNet(c["img_channels"], c["img_size"])
        model, net = bl.SiameseNet(enc, enc.embedding_dim), enc
    else:
        model = bl.ArcFace(bl.Backbone(c["num_layers"], 0.6, 'ir_se', c["img_size"], c["img_channels"]), 512, c["n_classes"])
        net = model.emb_model
    model.load_state_dict(bf.filled_state(entries, "bench/%s/" % cfg, torch.float32), strict=True)
    model.to(dev).train(mode=False)
    return net, (c["img_channels"], c["img_size"], c["img_size"])


def time_layers(counted, dev, reps=20):
    """[{shape, launches per forward, ms, TFLOP/s}] for the ("infer", (N, Ho, Wo, Cin, Cout, KH, stride)) entries of a count_flops dict."""
    rows = []
    for (kind, key), (launches, flops) in sorted(counted.items(), key=lambda kv: -kv[1][0] * kv[1][1]):
        if kind != "infer":
            continue
        N, Ho, Wo, Cin, Cout, KH, stride = key
        x = torch.randn(N, Ho * stride, Wo * stride, Cin, device=dev)
        w = torch.randn(Cout, KH, KH, Cin, device=dev) / (Cin * KH * KH) ** 0.5
        b, a = torch.randn(Cout, device=dev), torch.rand(Cout, device=dev) * 0.3
        with torch.no_grad():
            for _ in range(3):
                ops.conv2d_infer(x, w, b, a, stride)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(reps):
                ops.conv2d_infer(x, w, b, a, stride)
            t1.record()
            t1.synchronize()
        ms = t0.elapsed_time(t1) / reps
        rows.append({"N,Ho,Wo,Cin,Cout,K,stride": ",".join(map(str, key)), "launches": launches, "gflop": round(flops / 1e9, 3),
                     "ms": round(ms, 4), "tflops": round(flops / (ms * 1e-3) / 1e12, 1)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", action="store_true")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    if a.steps < 50:
        ap.error("--steps must be at least 50")
    dev = torch.device("cuda:0")
    cases = []
    for cfg in ("arcface50_64_3", "siamese_32_1"):
        net, img = build(cfg, dev)
        for n_img in (128, 512):
            x = torch.rand((n_img,) + img, device=dev) * 2 - 1
            with ops.count_flops() as c:
                net(x)
            flops = sum(v[0] * v[1] for v in c.values())
            launches = sum(v[0] for v in c.values())
            for _ in range(a.warmup):
                net(x)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.steps):
                net(x)
            t1.record()
            t1.synchronize()
            ms = t0.elapsed_time(t1) / a.steps
            cases.append({"net": cfg, "images": n_img, "ms_per_forward": round(ms, 4), "images_per_s": round(n_img / ms * 1e3, 1),
                          "conv_launches": launches, "conv_gflop_per_forward": round(flops / 1e9, 3),
                          "conv_flops_over_fp32_mfma_peak": round(flops / (ms * 1e-3) / PEAK_FP32_MFMA, 4)})
            if a.layers:
                cases[-1]["layers"] = time_layers(c, dev)
    print(json.dumps({"tool": "baseline_infer_bench", "steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
                      "peak_fp32_mfma_tflops": PEAK_FP32_MFMA / 1e12, "cases": cases}))


if __name__ == "__main__":
    main()
