"""Write tests/golden/siamese_train.npz by IMPORTING THE REFERENCE's siamese model and training it with torch on the CPU.

Runs only where the reference tree is present (its path: argv[1] or $GIM_REFERENCE); never imported by a test or by the product.
The fixture holds recorded results only; weights, images and the synthetic bank are regenerated from names (tests/baseline_fill.py,
tests/siamese_fill.py, the key list of tests/golden/baseline_keys.json).  The reference has no training loop for this model: the
loop here is the plain one - BCE-with-logits on classify(*encode(cat([x1, x2])).chunk(2)) (ONE encoder pass over both inputs, as the
engine runs it, so the batch statistics are over 2B images), torch.optim.Adam(lr = 1e-3).

(a) protocol: 3 iterations at B = 4 pairs in fp64 - logits and loss per iteration, every parameter's gradient of iteration 0, the
    BatchNorms' running statistics after each iteration, every parameter after the third; the same run in fp32 gives floor/<name>,
    the reference's own fp32-vs-fp64 relative L2 deviation of each recorded quantity.
(b) curve: 40 iterations at B = 16 on the synthetic separable bank, pairs drawn by the product's PairSampler (host logic) - the drawn
    indices and flips, loss and accuracy per iteration in fp64 and fp32, and |fp32 - fp64| of every 8-iteration window mean.

    python tools/make_siamese_train_golden.py /path/to/reference
"""
import json
import os
import sys

sys.dont_write_bytecode = True

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("GIM_REFERENCE", "")
if not os.path.isdir(os.path.join(REF, "baselines")):
    raise SystemExit("reference tree not found: pass its path")
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

from tests import baseline_fill as bf  # noqa: E402
from tests import siamese_fill as sf  # noqa: E402
from baselines.siamese.models import ProtonetEmbeddingNet, SiameseNet  # noqa: E402
from optimalstrategiesagainstgenerativeattacks_amd.baseline_training import PairSampler  # noqa: E402


def build(tag, dtype):
    with open(os.path.join(OUT, "baseline_keys.json")) as f:
        keys = json.load(f)["keys"][sf.CFG]
    enc = ProtonetEmbeddingNet(1, 32)
    model = SiameseNet(enc, enc.embedding_dim).to(dtype)
    model.load_state_dict(bf.filled_state(keys, tag, dtype), strict=True)
    return model.train()


def step(model, opt, x1, x2, n_pos):
    logits = model.classify(*model.encode(torch.cat([x1, x2], 0)).chunk(2))
    target = (torch.arange(x1.shape[0]) < n_pos).to(logits.dtype)
    loss = F.binary_cross_entropy_with_logits(logits.view(-1), target)
    opt.zero_grad()
    loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    opt.step()
    acc = ((logits.detach().view(-1) >= 0) == (target > 0.5)).double().mean()
    return logits.detach(), loss.detach(), acc, grads


def protocol(dtype):
    model = build(sf.PROTO_TAG, dtype)
    opt = torch.optim.Adam(model.parameters(), lr=sf.LR)
    rec = {}
    for it in range(sf.PROTO_ITERS):
        x1, x2 = (bf.images("%s%s/it%d" % (sf.PROTO_TAG, nm, it), (sf.PROTO_B, 1, 32, 32), dtype) for nm in ("x1", "x2"))
        logits, loss, _, grads = step(model, opt, x1, x2, sf.PROTO_N_POS)
        rec["it%d/logits" % it], rec["it%d/loss" % it] = logits, loss
        if it == 0:
            rec.update({"grad/" + k: g for k, g in grads.items()})
        for k, v in model.state_dict().items():
            if k.endswith(("running_mean", "running_var", "num_batches_tracked")):
                rec["it%d/%s" % (it, k)] = v.detach().clone()
    rec.update({"final/" + k: p.detach().clone() for k, p in model.named_parameters()})
    return rec


def curve(dtype, imgs, draws):
    model = build(sf.CURVE_TAG, dtype)
    opt = torch.optim.Adam(model.parameters(), lr=sf.LR)
    losses, accs, margin = [], [], np.inf
    for idx, flip in draws:
        x = torch.from_numpy(sf.gather_host(imgs, idx.T, flip.T)).to(dtype)
        logits, loss, acc, _ = step(model, opt, x[:sf.CURVE_B], x[sf.CURVE_B:], sf.CURVE_B // 2)
        losses.append(float(loss))
        accs.append(float(acc))
        margin = min(margin, float(logits.abs().min()))
    return np.array(losses), np.array(accs), margin


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm()) if float(b.norm()) > 0 else float((a - b).norm())


class _Offsets:
    """What PairSampler reads of a bank."""

    def __init__(self, offsets, mirror):
        self.offsets, self.mirror = offsets, mirror


def main():
    torch.set_num_threads(1)     # one summation order: the file regenerates byte for byte
    out = {}
    r64, r32 = protocol(torch.float64), protocol(torch.float32)
    for k, v in r64.items():
        if k.endswith("num_batches_tracked"):
            out[k] = v.numpy()
            continue
        big = k.startswith(("grad/", "final/"))
        out[k] = v.numpy().astype(np.float32) if big else v.numpy()
        out["floor/" + k] = np.float64(rel(r32[k], v))
    imgs, offsets = sf.separable_bank()
    sampler = PairSampler(_Offsets(offsets, True), sf.CURVE_B, sf.CURVE_SEED)
    draws = [sampler.draw(it)[:2] for it in range(sf.CURVE_ITERS)]
    l64, a64, m64 = curve(torch.float64, imgs, draws)
    l32, a32, m32 = curve(torch.float32, imgs, draws)
    assert min(m64, m32) >= 1e-2 and np.array_equal(a64, a32), "curve logits too close to the decision threshold 0: pick another CURVE_SEED"
    out.update({"curve/idx": np.stack([d[0] for d in draws]), "curve/flip": np.stack([d[1] for d in draws]),
                "curve/loss": l64, "curve/acc": a64, "curve/loss_f32": l32, "curve/acc_f32": a32,
                "curve/env_loss": np.abs(sf.window_means(l32) - sf.window_means(l64)),
                "curve/env_acc": np.abs(sf.window_means(a32) - sf.window_means(a64)),
                "curve/min_abs_logit": np.array([m64, m32])})
    np.savez_compressed(os.path.join(OUT, "siamese_train.npz"), **out)
    print("protocol losses", [float(r64["it%d/loss" % i]) for i in range(sf.PROTO_ITERS)])
    print("protocol logits it0", r64["it0/logits"].view(-1).tolist())
    print("largest floors", sorted(((float(v), k) for k, v in out.items() if k.startswith("floor/")), reverse=True)[:8])
    print("curve loss", np.round(l64, 4).tolist())
    print("curve acc", a64.tolist())
    print("curve env loss max %.3e acc max %.3e; min |logit| fp64 %.3e fp32 %.3e" % (out["curve/env_loss"].max(), out["curve/env_acc"].max(), m64, m32))
    print("file bytes", os.path.getsize(os.path.join(OUT, "siamese_train.npz")))


if __name__ == "__main__":
    main()
