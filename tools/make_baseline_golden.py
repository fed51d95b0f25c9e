"""Write tests/golden/baseline_keys.json and tests/golden/baselines.npz by IMPORTING THE REFERENCE's baseline models.

Runs only where the reference tree is present (its path: argv[1] or $GIM_REFERENCE); never imported by a test or by the product.
The fixtures hold key lists and OUTPUTS only (computed in fp64; whole-net quantities stored in fp64, plus the reference's own fp32 run of the whole-net quantities, so that they
carry the reference's fp32-vs-fp64 distance); weights and images are regenerated from names by tests/baseline_fill.py.

    python tools/make_baseline_golden.py /path/to/reference
"""
import json
import os
import sys

sys.dont_write_bytecode = True

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("GIM_REFERENCE", "")
if not os.path.isdir(os.path.join(REF, "baselines")):
    raise SystemExit("reference tree not found: pass its path")
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

from tests import baseline_fill as bf  # noqa: E402
from baselines.siamese.models import ProtonetEmbeddingNet, SiameseNet  # noqa: E402
from baselines.arcface.models import ArcFace, Backbone, bottleneck_IR_SE  # noqa: E402


def entry_kinds(model):
    kinds = {}
    for name, mod in model.named_modules():
        pre = name + "." if name else ""
        if isinstance(mod, nn.modules.batchnorm._BatchNorm):
            for leaf in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked"):
                kinds[pre + leaf] = "bn." + leaf
        elif isinstance(mod, nn.PReLU):
            kinds[pre + "weight"] = "prelu"
    return [[k, list(v.shape), "head" if k == "head.kernel" else kinds.get(k, "other")] for k, v in model.state_dict().items()]


def build(cfg):
    c = bf.CONFIGS[cfg]
    if c["kind"] == "siamese":
        enc = ProtonetEmbeddingNet(c["img_channels"], c["img_size"])
        return SiameseNet(enc, enc.embedding_dim)
    return ArcFace(Backbone(c["num_layers"], 0.6, 'ir_se', c["img_size"], c["img_channels"]), 512, c["n_classes"])


# the reference's agent wrappers (eval_gim_on_authentication.py imports pandas and the datasets at module level; the two
# closures are re-stated here on the reference's MODELS - this file is a generator, not product code)
def siamese_au(model, test, si):
    model.train(mode=False)
    with torch.no_grad():
        B, k = si.shape[:2]
        n = test.shape[1]
        si_emb = model.encode(si.reshape(B * k, *si.shape[2:])).view(B, k, -1).mean(dim=1)
        test_emb = model.encode(test.reshape(B * n, *test.shape[2:])).view(B, n, -1).mean(dim=1)
        return model.classify(si_emb, test_emb).squeeze()


def arcface_au(arc, test, si):
    arc.train(mode=False)
    with torch.no_grad():
        return arc.predict(x1=test.mean(1), x2=si.mean(1))[0]


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def _f32(t):
    """Block outputs are COMPUTED in fp64 and stored rounded to fp32 (3e-8 relative, against a parity bound of 1e-3): in fp64
    the (128, 128, 1) unit's 16x16 output alone is 0.8 MB, and the two fixture files have to stay under 1 MB together."""
    return t.numpy().astype(np.float32)


def main():
    keys, out, meta = {}, {}, {"fp32_vs_fp64": {}}
    for cfg in bf.CONFIGS:
        keys[cfg] = entry_kinds(build(cfg))

    # (i) one siamese conv block, (ii) three IR-SE units: sub-modules filled under their names inside the whole net
    tag = "bl/siamese_32_1/"
    sia = build("siamese_32_1").double()
    sia.load_state_dict(bf.filled_state(keys["siamese_32_1"], tag), strict=True)
    sia.train(mode=False)
    with torch.no_grad():
        out["block_conv"] = _f32(sia.embedding_net.encoder[1](bf.images("bl/block_conv/x", (3, 64, 16, 16))))
    unit_entries = {}
    for (cin, depth, stride), body_idx in (((64, 64, 2), 0), ((64, 128, 2), 3), ((128, 128, 1), 4)):
        pre = "emb_model.body.%d." % body_idx
        ent = [e for e in keys["arcface50_64_3"] if e[0].startswith(pre)]
        unit = bottleneck_IR_SE(cin, depth, stride).double()
        unit.load_state_dict(bf.filled_state(ent, "bl/arcface50_64_3/", prefix=pre), strict=True)
        unit.train(mode=False)
        name = "unit_%d_%d_%d" % (cin, depth, stride)
        with torch.no_grad():
            out[name] = _f32(unit(bf.images("bl/%s/x" % name, (3, cin, 16, 16))))
        unit_entries[name] = body_idx
    meta["unit_body_index"] = unit_entries

    # (iii) siamese: embeddings and logits, B = 4, n = 5, k = 3
    B, n, k = 4, 5, 3
    test, si = bf.images(tag + "test", (B, n, 1, 32, 32)), bf.images(tag + "si", (B, k, 1, 32, 32))
    with torch.no_grad():
        e64 = sia.encode(test.reshape(B * n, 1, 32, 32))
    l64 = siamese_au(sia, test, si)
    sia32 = build("siamese_32_1")
    sia32.load_state_dict(bf.filled_state(keys["siamese_32_1"], tag, torch.float32), strict=True)
    sia32.train(mode=False)
    with torch.no_grad():
        e32 = sia32.encode(test.float().reshape(B * n, 1, 32, 32))
    l32 = siamese_au(sia32, test.float(), si.float())
    out.update(siamese_emb=e64.numpy(), siamese_logits=l64.numpy(), siamese_emb_f32=e32.numpy(), siamese_logits_f32=l32.numpy())
    meta["fp32_vs_fp64"].update(siamese_emb=rel(e32, e64), siamese_logits=rel(l32, l64))
    print("siamese logits", l64.tolist())
    assert min(float(l64.abs().min()), float(l32.abs().min())) >= 1e-2 and torch.equal(l64 >= 0, l32 >= 0), "siamese logits too close to the decision threshold 0"

    # (iv) ArcFace-50: embeddings of 4 images, scores for B = 4, n = 5, k = 5
    for cfg in ("arcface50_64_3", "arcface50_32_1"):
        c = bf.CONFIGS[cfg]
        S, C = c["img_size"], c["img_channels"]
        tag = "bl/%s/" % cfg
        x = bf.images(tag + "x", (4, C, S, S))
        test, si = bf.images(tag + "test", (4, 5, C, S, S)), bf.images(tag + "si", (4, 5, C, S, S))
        res = {}
        for dt in (torch.float64, torch.float32):
            arc = build(cfg).to(dt)
            arc.load_state_dict(bf.filled_state(keys[cfg], tag, dt), strict=True)
            arc.train(mode=False)
            with torch.no_grad():
                res[dt] = (arc.emb_model(x.to(dt)), arcface_au(arc, test.to(dt), si.to(dt)))
            del arc
        (e64, s64), (e32, s32) = res[torch.float64], res[torch.float32]
        out.update({cfg + "_emb": e64.numpy(), cfg + "_score": s64.numpy(), cfg + "_emb_f32": e32.numpy(), cfg + "_score_f32": s32.numpy()})
        meta["fp32_vs_fp64"].update({cfg + "_emb": rel(e32, e64), cfg + "_score": rel(s32, s64)})
        # threshold: midpoint of the widest gap between neighbouring fp64 scores; every score at least 1e-2 away from it
        srt = np.sort(s64.numpy())
        i = int(np.argmax(np.diff(srt)))
        th = float(0.5 * (srt[i] + srt[i + 1]))
        assert min(float(np.abs(s64.numpy() - th).min()), float(np.abs(s32.numpy() - th).min())) >= 1e-2, (cfg, srt, th)
        meta[cfg + "_th"] = th
        meta[cfg + "_emb_absmax"] = float(e64.abs().max())
        meta[cfg + "_scores"] = [float(v) for v in s64]
        meta[cfg + "_n_params"] = int(sum(int(np.prod(s)) for _, s, kd in keys[cfg] if kd != "bn.num_batches_tracked"))
    with open(os.path.join(OUT, "baseline_keys.json"), "w") as f:
        json.dump({"keys": keys, "meta": meta}, f)
    np.savez_compressed(os.path.join(OUT, "baselines.npz"), **out)
    print(json.dumps(meta, indent=1))


if __name__ == "__main__":
    main()
