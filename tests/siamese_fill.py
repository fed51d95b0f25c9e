"""What tools/make_siamese_train_golden.py and the siamese training tests share: the names the fixture's weights and images are
regenerated from, the protocol's sizes, and the synthetic separable image bank (a rule over names, nothing is committed)."""
import numpy as np

from oracle import portable_fill as pf

CFG = "siamese_32_1"                 # key list in tests/golden/baseline_keys.json
LR = 1e-3

# (a) three-step protocol: B pairs of 32x32x1 images, the first N_POS of them same-class pairs
PROTO_TAG = "bl/siamese_train/"
PROTO_B, PROTO_N_POS, PROTO_ITERS = 4, 2, 3

# (b) loss curve on the synthetic bank
CURVE_TAG = "bl/siamese_curve/"
# (CURVE_SEED: a sampler seed for which every logit of the reference's fp64 and fp32 runs stays >= 1e-2 away from the decision
# threshold 0 - the tool asserts it - so that the accuracy curve does not hang on a rounding)
CURVE_B, CURVE_ITERS, CURVE_SEED, WINDOW = 16, 40, 3, 8
BANK_CLASSES, BANK_PER_CLASS, BANK_S = 8, 6, 32


def separable_bank(n_classes=BANK_CLASSES, per_class=BANK_PER_CLASS, S=BANK_S):
    """(uint8 [n_classes * per_class, S, S, 1], class offsets): a blocky left-right symmetric prototype per class (a horizontal flip
    keeps the class) plus per-image noise."""
    imgs = np.empty((n_classes * per_class, S, S, 1), dtype=np.uint8)
    for c in range(n_classes):
        p = pf.uniform("sia/bank/proto/%d" % c, (S // 4, S // 4))
        proto = np.kron(0.5 * (p + p[:, ::-1]), np.ones((4, 4)))
        for i in range(per_class):
            v = 127.5 + 90.0 * proto + 25.0 * pf.normal("sia/bank/img/%d/%d" % (c, i), (S, S))
            imgs[c * per_class + i, :, :, 0] = np.clip(np.rint(v), 0, 255).astype(np.uint8)
    return imgs, np.arange(n_classes + 1) * per_class


def gather_host(imgs, idx, flip):
    """data.EpisodeBank.gather on the host, in the kernel's fp32 arithmetic: float32 [len(idx), C, S, S] in [-1, 1]."""
    idx, flip = np.asarray(idx).reshape(-1), np.asarray(flip).reshape(-1)
    x = imgs[idx]
    x = np.where(flip[:, None, None, None].astype(bool), x[:, :, ::-1], x).astype(np.float32)
    x = ((x / np.float32(255.0)) * np.float32(2.0) + np.float32(-1.0)).transpose(0, 3, 1, 2)
    return np.array(x, order="C").reshape(x.shape)      # (canonical strides also for C = 1)


def window_means(v, w=WINDOW):
    """Means of every window of w consecutive iterations."""
    v = np.asarray(v, dtype=np.float64)
    c = np.concatenate([[0.0], np.cumsum(v)])
    return (c[w:] - c[:-w]) / w
