"""Fill rules for the baseline authenticators' state dicts, on top of ``oracle.portable_fill`` (imported, not edited).

The KIND of an entry (BatchNorm / PReLU / the ArcFace head / anything else) cannot be told from its key, so the key fixture
``tests/golden/baseline_keys.json`` carries it: ``[key, shape, kind]`` with kind in
``bn.weight | bn.bias | bn.running_mean | bn.running_var | bn.num_batches_tracked | prelu | head | other``.
Weights are regenerated from names wherever they are needed (ArcFace-50 has 32 M parameters: they are never committed)."""
import numpy as np
import torch

from oracle import portable_fill as pf


def fill_entry(key, shape, kind, tag):
    shape = tuple(shape)
    if kind == "bn.num_batches_tracked":
        return np.array(7, dtype=np.int64)
    if kind == "other":
        return pf.fill_value(key, shape, tag)
    u = pf.uniform(tag + key, shape)
    if kind == "bn.weight":
        return 1.0 + 0.3 * u
    if kind == "bn.bias":
        return 0.3 * u
    if kind == "bn.running_mean":
        return 0.2 * u
    if kind == "bn.running_var":
        return 1.0 + 0.5 * np.abs(u)
    if kind == "prelu":
        return 0.25 * (1.0 + 0.5 * u)
    if kind == "head":
        return u
    raise KeyError("no fill rule for kind %s (%s)" % (kind, key))


def filled_state(entries, tag, dtype=torch.float64, prefix=""):
    """Ordered {key: tensor} for the ``[key, shape, kind]`` entries whose key starts with ``prefix`` (stripped from the result; the
    fill is keyed by the FULL key, so a sub-module's values equal its values inside the whole net)."""
    out = {}
    for key, shape, kind in entries:
        if not key.startswith(prefix):
            continue
        v = torch.from_numpy(np.ascontiguousarray(fill_entry(key, shape, kind, tag)))
        out[key[len(prefix):]] = v if kind == "bn.num_batches_tracked" else v.to(dtype)
    return out


def images(tag, shape, dtype=torch.float64):
    """Images as tests.helpers.episode makes them: clip(0.5 * normal, -1, 1)."""
    return torch.from_numpy(np.clip(pf.normal(tag, tuple(shape)) * 0.5, -1, 1)).to(dtype)


CONFIGS = {
    "siamese_32_1": dict(kind="siamese", img_size=32, img_channels=1),
    "arcface50_64_3": dict(kind="arcface", num_layers=50, img_size=64, img_channels=3, n_classes=11),
    "arcface50_32_1": dict(kind="arcface", num_layers=50, img_size=32, img_channels=1, n_classes=11),
}
