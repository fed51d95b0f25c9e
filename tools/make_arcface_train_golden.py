"""Write tests/golden/arcface_train.npz by IMPORTING THE REFERENCE's ArcFace model and training it with torch on the CPU.

Runs only where the reference tree is present (its path: argv[1] or $GIM_REFERENCE); never imported by a test or by the product.
The fixture holds recorded results only; weights, images and the synthetic bank are regenerated from names (tests/baseline_fill.py,
tests/arcface_fill.py, tests/siamese_fill.py, the key list of tests/golden/baseline_keys.json).  The reference has no training loop
for this model: the loop here is the plain one - cross-entropy on ``ArcFace.forward(x, label)[1]``, ``torch.optim.Adam``.  ArcFace-50
has 32 M parameters, so every gradient / update tensor is stored as <= 256 strided elements (updates: every second one of them) (arcface_fill.sample_index)
plus its fp64 norm.  Every recorded quantity q has floor/q, the reference's own fp32-vs-fp64 relative L2 deviation.

(a) units: bottleneck_IR_SE in training mode at (64, 64, 2), (64, 128, 2), (128, 128, 1), N = 4, 8 x 8, fp64: output, input gradient
    for a seeded cotangent, every parameter gradient (sampled), the running statistics after the pass.
(b) protocol: ArcFace(Backbone(50, 0.0, 'ir_se', 32, 1), 512, 11), B = 8, labels (3 i) mod 11, Adam(lr = 1e-5), 3 iterations: emb,
    logits, loss and five BatchNorms' running statistics per iteration; at iteration 0 every parameter's gradient samples and norm
    and its update.  lr stays this small on purpose: Adam turns rounding noise into +-lr steps, at 1e-4 the reference's own fp32
    gradients of iterations 1 and 2 are 1e-2 off its fp64 run.
(c) curve: 24 iterations at B = 16, lr = 1e-4 on the synthetic separable bank (8 classes, head width 8), drawn by the product's
    IdentitySampler (host logic): loss and top-1 accuracy in fp64 and fp32, |fp32 - fp64| of every 8-iteration window mean.

The conditions the tests rely on are asserted here, on the reference alone.

    python tools/make_arcface_train_golden.py /path/to/reference
"""
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

from tests import arcface_fill as af  # noqa: E402
from tests import baseline_fill as bf  # noqa: E402
from tests import siamese_fill as sf  # noqa: E402
from baselines.arcface.models import ArcFace, Backbone, bottleneck_IR_SE  # noqa: E402
from optimalstrategiesagainstgenerativeattacks_amd.baseline_training import IdentitySampler  # noqa: E402

FLOOR_CAP = 3e-5


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm()) if float(b.norm()) > 0 else float((a - b).norm())


def sampled(t, index=af.sample_index):
    return t.detach().reshape(-1)[torch.from_numpy(index(t.numel()))]


# ---------------------------------------------------------------------------------------------------- (a)
def unit_pass(cin, depth, stride, body_idx, dtype):
    ent, pre = af.unit_entries(body_idx)
    unit = bottleneck_IR_SE(cin, depth, stride).to(dtype)
    unit.load_state_dict(bf.filled_state(ent, af.UNIT_TAG, dtype, prefix=pre), strict=True)
    unit.train()
    x, dy = af.unit_input(cin, depth, stride)
    x = torch.from_numpy(x).to(dtype).requires_grad_()
    out = unit(x)
    out.backward(torch.from_numpy(dy).to(dtype))
    name = af.unit_name(cin, depth, stride)
    rec = {name + "/out": out.detach(), name + "/dx": x.grad.detach()}
    for k, p in unit.named_parameters():
        rec["%s/grad/%s" % (name, k)] = p.grad.detach()
    for k, v in unit.state_dict().items():
        if k.endswith(("running_mean", "running_var")):
            rec["%s/run/%s" % (name, k)] = v.detach().clone()
    return rec


# ---------------------------------------------------------------------------------------------------- (b)
def build(tag, dtype, n_classes):
    model = ArcFace(Backbone(af.NUM_LAYERS, 0.0, 'ir_se', af.IMG_SIZE, af.IMG_CHANNELS), af.EMB_DIM, n_classes).to(dtype)
    model.load_state_dict(bf.filled_state(af.keys(n_classes), tag, dtype), strict=True)
    return model.train()


def protocol(dtype):
    model = build(af.PROTO_TAG, dtype, af.PROTO_CLASSES)
    opt = torch.optim.Adam(model.parameters(), lr=af.PROTO_LR)
    label = torch.from_numpy(af.proto_labels())
    rec = {}
    for it in range(af.PROTO_ITERS):
        x = torch.from_numpy(af.proto_images(it)).to(dtype)
        emb, logits = model(x, label)
        loss = F.cross_entropy(logits, label)
        opt.zero_grad()
        loss.backward()
        rec["it%d/emb" % it], rec["it%d/logits" % it], rec["it%d/loss" % it] = emb.detach(), logits.detach(), loss.detach()
        if it == 0:
            before = {k: p.detach().clone() for k, p in model.named_parameters()}
            rec.update({"grad/" + k: p.grad.detach().clone() for k, p in model.named_parameters()})
        opt.step()
        if it == 0:
            rec.update({"delta/" + k: (p.detach() - before[k]) for k, p in model.named_parameters()})
        sd = model.state_dict()
        for bn in af.RUNNING:
            for leaf in ("running_mean", "running_var"):
                rec["it%d/run/%s.%s" % (it, bn, leaf)] = sd["emb_model.%s.%s" % (bn, leaf)].detach().clone()
        print("protocol", dtype, "iteration", it, "loss", float(loss), flush=True)
    return rec


# ---------------------------------------------------------------------------------------------------- (c)
class _Offsets:
    """What IdentitySampler reads of a bank."""

    def __init__(self, offsets, mirror):
        self.offsets, self.mirror = offsets, mirror


def curve(dtype, imgs, draws):
    model = build(af.CURVE_TAG, dtype, af.CURVE_CLASSES)
    opt = torch.optim.Adam(model.parameters(), lr=af.CURVE_LR)
    losses, accs = [], []
    for idx, flip, label in draws:
        x = torch.from_numpy(sf.gather_host(imgs, idx, flip)).to(dtype)
        label = torch.from_numpy(label)
        _, logits = model(x, label)
        loss = F.cross_entropy(logits, label)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss))
        accs.append(float((logits.detach().argmax(1) == label).double().mean()))
        print("curve", dtype, len(losses), losses[-1], accs[-1], flush=True)
    return np.array(losses), np.array(accs)


def main():
    torch.set_num_threads(1)     # one summation order: the file regenerates byte for byte
    out = {}

    # (a)
    worst_run = 0.0
    for cin, depth, stride, body_idx in af.UNITS:
        r64, r32 = unit_pass(cin, depth, stride, body_idx, torch.float64), unit_pass(cin, depth, stride, body_idx, torch.float32)
        for k, v in r64.items():
            out["floor/" + k] = np.float64(rel(r32[k], v))
            if "/grad/" in k:
                out[k] = sampled(v).numpy().astype(np.float32)
                out[k.replace("/grad/", "/gradnorm/")] = np.float64(v.norm())
            elif "/run/" in k:
                out[k] = v.numpy()
                worst_run = max(worst_run, float(out["floor/" + k]))
            else:
                out[k] = v.numpy().astype(np.float32)      # computed in fp64, stored rounded (6e-8 relative)
        print(af.unit_name(cin, depth, stride), "largest floor", max(float(out["floor/" + k]) for k in r64))

    # (b)
    r64, r32 = protocol(torch.float64), protocol(torch.float32)
    names = [k[len("grad/"):] for k in r64 if k.startswith("grad/")]
    norms = {k: float(r64["grad/" + k].norm()) for k in names}
    largest = max(norms.values())
    small = [k for k in names if norms[k] < af.SMALL_REL * largest]
    assert len(small) <= 10, small
    print("small tensors:", [(k, norms[k] / largest, float(r32["grad/" + k].double().norm()) / largest) for k in small])
    masked = total = 0
    worst_update = 0.0
    packed = {"grad": [], "delta": [], "gradnorm": [], "floor_grad": []}
    for name in names:      # one packed array per kind, in parameter order (arcface_fill.unpack): 236 tensors, four entries
        g64, d64 = r64["grad/" + name], r64["delta/" + name]
        f = rel(r32["grad/" + name], g64)
        packed["grad"].append(sampled(g64).numpy().astype(np.float32))
        packed["delta"].append(sampled(d64, af.delta_index).numpy().astype(np.float32))
        packed["gradnorm"].append(norms[name])
        packed["floor_grad"].append(f)
        if name in small:
            continue
        assert f <= FLOOR_CAP, (name, f)
        # the update check of the GPU test, on the reference's own fp32 run
        g = sampled(g64, af.delta_index)
        keep = g.abs() >= af.MASK_REL * norms[name] / np.sqrt(g64.numel())
        masked += int((~keep).sum())
        total += keep.numel()
        d = (sampled(r32["delta/" + name], af.delta_index).double() - sampled(d64, af.delta_index))[keep].abs()
        worst_update = max(worst_update, float(d.max()) if d.numel() else 0.0)
    out.update(grad=np.concatenate(packed["grad"]), delta=np.concatenate(packed["delta"]), gradnorm=np.array(packed["gradnorm"]),
               floor_grad=np.array(packed["floor_grad"]), grad_names=np.array(names))
    for k, v in r64.items():
        if k.startswith(("grad/", "delta/")):
            continue
        f = rel(r32[k], v)
        out["floor/" + k] = np.float64(f)
        if "/run/" in k:
            out[k] = v.numpy()
            worst_run = max(worst_run, f)
        else:
            out[k] = v.numpy().astype(np.float32) if k.endswith("/emb") else v.numpy()
            assert f <= FLOOR_CAP, (k, f)
    out["small"] = np.array(small)
    share = masked / total
    print("masked share of the sampled update elements %.4f; worst |dp32 - dp64| on the rest %.3e (0.1 lr = %.1e)"
          % (share, worst_update, 0.1 * af.PROTO_LR))
    assert share <= 0.05 and worst_update <= 0.1 * af.PROTO_LR
    out["masked_share"], out["worst_update_f32"] = np.float64(share), np.float64(worst_update)
    print("largest running-statistics floor %.3e" % worst_run)
    print("largest floors", sorted(((float(v), k) for k, v in out.items() if k.startswith("floor/")), reverse=True)[:8])

    # (c)
    imgs, offsets = sf.separable_bank()
    sampler = IdentitySampler(_Offsets(offsets, True), af.CURVE_B, af.CURVE_SEED)
    draws = [sampler.draw(it) for it in range(af.CURVE_ITERS)]
    l64, a64 = curve(torch.float64, imgs, draws)
    l32, a32 = curve(torch.float32, imgs, draws)
    env_loss = np.abs(sf.window_means(l32, af.WINDOW) - sf.window_means(l64, af.WINDOW))
    env_acc = np.abs(sf.window_means(a32, af.WINDOW) - sf.window_means(a64, af.WINDOW))
    first = sf.window_means(l64, af.WINDOW)[0]
    print("curve loss", np.round(l64, 4).tolist())
    print("curve acc", a64.tolist())
    print("curve env loss max %.3e against a first window mean of %.3f; env acc max %.3e" % (env_loss.max(), first, env_acc.max()))
    assert env_loss.max() <= 0.01 * first
    out.update({"curve/idx": np.stack([d[0] for d in draws]), "curve/flip": np.stack([d[1] for d in draws]),
                "curve/label": np.stack([d[2] for d in draws]), "curve/loss": l64, "curve/acc": a64, "curve/loss_f32": l32,
                "curve/acc_f32": a32, "curve/env_loss": env_loss, "curve/env_acc": env_acc})
    path = os.path.join(OUT, "arcface_train.npz")
    np.savez_compressed(path, **out)
    print("file bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
