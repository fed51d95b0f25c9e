"""What tools/make_arcface_train_golden.py and the ArcFace training tests share: the names the fixture's weights and images are
regenerated from, the protocol's sizes and the sampling rule of the large tensors (nothing here is committed as data)."""
import json
import os

import numpy as np

from oracle import portable_fill as pf
from tests import baseline_fill as bf

CFG = "arcface50_32_1"               # key list in tests/golden/baseline_keys.json
NUM_LAYERS, IMG_SIZE, IMG_CHANNELS, EMB_DIM = 50, 32, 1, 512

# (a) units in training mode: (in_channel, depth, stride, index in the body whose names the fill is keyed by)
UNIT_TAG = "bl/arcface_unit/"
UNITS = ((64, 64, 2, 0), (64, 128, 2, 3), (128, 128, 1, 4))
UNIT_N, UNIT_HW = 4, 8

# (b) three-step protocol
PROTO_TAG = "bl/arcface_train/"
PROTO_B, PROTO_ITERS, PROTO_CLASSES, PROTO_LR = 8, 3, 11, 1e-5
RUNNING = ("input_layer.1", "body.0.res_layer.0", "body.23.res_layer.4", "output_layer.0", "output_layer.4")
SMALL_REL = 1e-6        # a gradient tensor is "small" when its fp64 norm is below this share of the largest tensor's
MASK_REL = 1e-3         # elements with |g| < MASK_REL * rms(g) are left out of the update check (Adam amplifies their rounding)
SAMPLES = 256         # stored elements of a gradient tensor; its update is stored at every second one of them

# (c) loss curve on the synthetic bank of tests/siamese_fill.py
CURVE_TAG = "bl/arcface_curve/"
CURVE_B, CURVE_ITERS, CURVE_LR, CURVE_SEED, CURVE_CLASSES, WINDOW = 16, 24, 1e-4, 3, 8, 8

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def keys(n_classes=PROTO_CLASSES):
    """[key, shape, kind] of ArcFace-50 on 32 x 32 x 1 images with a head of n_classes columns."""
    with open(os.path.join(GOLDEN, "baseline_keys.json")) as f:
        ent = json.load(f)["keys"][CFG]
    return [[k, ([EMB_DIM, n_classes] if k == "head.kernel" else s), kind] for k, s, kind in ent]


def unit_name(cin, depth, stride):
    return "unit_%d_%d_%d" % (cin, depth, stride)


def unit_entries(body_idx):
    pre = "emb_model.body.%d." % body_idx
    return [e for e in keys() if e[0].startswith(pre)], pre


def unit_input(cin, depth, stride):
    """(x [N, cin, HW, HW], cotangent [N, depth, HW / stride, HW / stride]) in fp64 numpy, NCHW."""
    name = unit_name(cin, depth, stride)
    x = bf.images(UNIT_TAG + name + "/x", (UNIT_N, cin, UNIT_HW, UNIT_HW)).numpy()
    return x, pf.normal(UNIT_TAG + name + "/dy", (UNIT_N, depth, UNIT_HW // stride, UNIT_HW // stride))


def proto_labels():
    return (3 * np.arange(PROTO_B)) % PROTO_CLASSES


def proto_images(it):
    return bf.images("%sx/it%d" % (PROTO_TAG, it), (PROTO_B, IMG_CHANNELS, IMG_SIZE, IMG_SIZE)).numpy()


def sample_index(numel, n=SAMPLES):
    """At most n flat positions of a tensor of numel elements (its logical, reference layout), evenly strided by an odd step."""
    if numel <= n:
        return np.arange(numel)
    return (np.arange(n) * ((numel // n) | 1)) % numel


def delta_index(numel):
    """The positions at which a parameter's update is stored: every second gradient sample (so the reference gradient is known there)."""
    return sample_index(numel)[::2]


def parameter_entries(n_classes=PROTO_CLASSES):
    """[(name, numel)] of the parameters (not the buffers), in the reference's parameter order."""
    return [(k, int(np.prod(s))) for k, s, kind in keys(n_classes) if not kind.startswith("bn.running") and kind != "bn.num_batches_tracked"]


def unpack(packed, index=sample_index):
    """{name: samples} of one packed array of the fixture ("grad": sample_index, "delta": delta_index)."""
    out, off = {}, 0
    for name, numel in parameter_entries():
        m = len(index(numel))
        out[name] = packed[off:off + m]
        off += m
    assert off == len(packed)
    return out
