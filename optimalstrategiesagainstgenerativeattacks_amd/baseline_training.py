"""Training the siamese baseline authenticator (``baselines.SiameseNet``: ``baselines/siamese/models.py:14-56,97-114``) on the engine.

The reference ships the model but neither a training loop nor a checkpoint; its evaluation (``eval_gim_on_authentication.py:47-58``)
loads ``ckpts/model_*.pt['model']`` of an experiment directory with an ``args.json``.  ``train_siamese`` writes exactly that, so
``authentication_eval.eval_authentication_task(baseline_type='siamese', baseline_exp_dir=out_dir)`` runs on its output unchanged.

The training forward does not go through ``model.forward`` (the inference path on folded parameters, which keeps raising in training
mode): ``siamese_forward_train`` runs the four blocks as ``ops.conv2d`` + ``ops.bn_relu_maxpool2`` (BatchNorm with batch statistics,
ReLU and MaxPool2d(2) in one pass, csrc/bn_train.hip), brings the last map into the reference's (c, h, w) flatten order with the
existing NHWC -> NCHW kernel, then ``ops.absdiff_halves`` and ``ops.linear``.  Because the embedding is in the reference's order, every
parameter - ``fc.weight`` included - is trained in the reference's own layout: ``state_dict()`` has the reference's names, shapes, order
and values, with no permutation to undo.  (The inference path reads the (h, w, c) embedding and permutes the fc columns when it derives
its parameters, baselines.SiameseNet._derive.)

Both inputs of a pair batch go through the encoder in ONE pass, so the batch statistics are over 2B images:
``classify(*encode(cat([x1, x2])).chunk(2))`` on the reference's modules.  fp32 matrix path.

Data-parallel (one process per GPU under torch.distributed): BatchNorm with batch statistics is the only operator
of either baseline that couples the images of a batch.  With a `sync` (ops.DistSync) every BatchNorm takes its statistics and the two
sums of its backward over all ranks, the samplers hand each rank its slice of the global batch and the dropout hash is indexed by the
global element: the step of `world` ranks equals the single-process step on the whole batch.  Ranks exchange neither parameters nor
buffers - they stay equal because every rank merges the same gathered statistics in the same order and FusedAdam.step all-reduces
the gradient bucket.  Without a process group nothing changes.

The second half of the file trains the ArcFace baseline (``baselines.ArcFace`` on the IR-SE ``Backbone``: ``baselines/arcface/models.py``)
the same way: ``arcface_forward_train`` is the reference's ``ArcFace.forward(x, label)`` in training mode over the inference classes'
parameters (csrc/irse_train.hip for everything but the convolutions: ``ops.conv2d``, and ``ops.conv2d_strided`` for the stride-2 ones),
``train_arcface`` writes ``ckpts/model_*.pt['arcface']`` and the ``args.json`` that ``get_arcface_authenticator`` reads."""
import json
import os

import numpy as np
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib, ops
from ._lib import check
from .baselines import ArcFace, Backbone, ProtonetEmbeddingNet, SiameseNet
from .optim import FusedAdam
from .training_logger import Logger
from .training_utils import get_latest_ckpt

CHECKPOINT_DIR = "ckpts"


def _pair_batch(x1, x2):
    """[2B, C, S, S]: x1 on top of x2.  The two halves of one tensor (PairSampler.batch) are recognised and not copied."""
    if x1.shape != x2.shape:
        raise RuntimeError("siamese training: x1 %s and x2 %s differ in shape" % (tuple(x1.shape), tuple(x2.shape)))
    base = x1._base
    if (base is not None and base is x2._base and x1.is_contiguous() and x2.is_contiguous() and base.is_contiguous()
            and base.numel() == 2 * x1.numel() and base.data_ptr() == x1.data_ptr()
            and x2.data_ptr() == x1.data_ptr() + x1.numel() * x1.element_size()):
        return base.view(2 * x1.shape[0], *x1.shape[1:])
    return torch.cat([x1, x2], 0)


def _forward_pairs(model, x, sync=None):
    """Logits [B, 1] of the pair batch x = [x1; x2] ([2B, C, S, S]); sync: the rank's pairs of a data-parallel batch."""
    net = model.embedding_net
    dims = (net.inp_n_channels, net.inp_img_size, net.inp_img_size)
    x = ops._req(x, "x")
    if x.dim() != 4 or tuple(x.shape[1:]) != dims or x.shape[0] % 2:
        raise RuntimeError("expected [2B, %d, %d, %d] images, got %s" % (dims + (tuple(x.shape),)))
    h = ops.to_nhwc(x)
    for conv, bn in net.encoder:
        z = ops.conv2d(h, conv.weight, conv.bias)
        h = ops.bn_relu_maxpool2(z, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.momentum, bn.eps,
                                 sync)
    e = ops.to_nchw(h).view(h.shape[0], -1)      # the reference's (c, h, w) flatten order
    return ops.linear(ops.absdiff_halves(e), model.fc.weight, model.fc.bias)


def siamese_forward_train(model, x1, x2, sync=None):
    """Training-mode logits [B, 1] of a baselines.SiameseNet: batch statistics over the 2B images of one encoder pass, running
    statistics updated; differentiable in every parameter.  The model's ``training`` flag is neither read nor changed.
    sync (ops.DistSync): x1, x2 are this rank's equal share of the pairs, the statistics are over all ranks' images."""
    return _forward_pairs(model, _pair_batch(x1, x2), sync)


class _PairLossFn(Function):
    """(sum_{i < n_pos} bce(x_i, 1) + sum_{i >= n_pos} bce(x_i, 0)) / B as a [1] tensor: the BCE kernel with its scalar target on each
    half of the logits, then the row-sum kernel - and their transposes going back."""

    @staticmethod
    def forward(ctx, logits, n_pos):
        lib = _lib.load()
        x = ops._req(logits, "logits")
        B = x.numel()
        st = ops._stream()
        per = torch.empty(B, device=x.device, dtype=torch.float32)
        for off, n, target in ((0, n_pos, 1.0), (n_pos, B - n_pos, 0.0)):
            if n:
                check(lib.gim_bce_logits_fwd(ops._p(x, off), ops._p(per, off), target, n, st), "bce_logits_fwd")
        loss = torch.empty(1, device=x.device, dtype=torch.float32)
        check(lib.gim_sum_dim1(ops._p(per), ops._p(loss), 1, B, 1, 1.0 / B, st), "sum_dim1")
        ctx.save_for_backward(x)
        ctx.n_pos = n_pos
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, dl):
        lib = _lib.load()
        (x,) = ctx.saved_tensors
        B, n_pos = x.numel(), ctx.n_pos
        st = ops._stream()
        dl = ops._req(dl, "dloss")
        dper = torch.empty(B, device=x.device, dtype=torch.float32)
        check(lib.gim_repeat_dim1(ops._p(dl), ops._p(dper), 1, B, 1, 1.0 / B, st), "repeat_dim1")
        dx = torch.empty_like(x)
        for off, n, target in ((0, n_pos, 1.0), (n_pos, B - n_pos, 0.0)):
            if n:
                check(lib.gim_bce_logits_bwd(ops._p(dper, off), ops._p(x, off), ops._p(dx, off), target, n, st), "bce_logits_bwd")
        return dx, None


def pair_loss(logits, n_pos):
    """Mean BCE-with-logits of a pair batch whose first n_pos rows are same-class pairs (target 1), the rest target 0; a [1] tensor."""
    if not 0 <= n_pos <= logits.numel():
        raise ValueError("n_pos = %d outside [0, %d]" % (n_pos, logits.numel()))
    return _PairLossFn.apply(logits, n_pos)


def pair_accuracy(logits, n_pos):
    """Share of the logits on the right side of 0 (prediction: logit >= 0, as agents.Authenticator with th = 0); a device scalar."""
    x = ops._req(logits.detach(), "logits")
    out = torch.empty(1, device=x.device, dtype=torch.float32)
    check(_lib.load().gim_logit_accuracy(ops._p(x), n_pos, x.numel(), ops._p(out), ops._stream()), "logit_accuracy")
    return out.view(())


class _BaselineTrainer:
    """One FusedAdam over every parameter of a baseline model, in the reference's parameter order.  A subclass names its model class
    (MODEL) and supplies _loss_and_accuracy (the training forward; it may keep what it wants of it, as last_logits) and
    _inference_caches (the modules whose derived inference parameters an update makes stale).
    sync: how the BatchNorms reach the other ranks of a data-parallel run (ops.DistSync); None: over torch.distributed's default
    group when that is initialised with more than one rank, else a single process.  The gradient bucket is all-reduced by
    FusedAdam.step; the backward runs on the calling thread, so all ranks issue their collectives in one order."""

    MODEL = None

    def __init__(self, model, lr, betas, sync=None):
        if not isinstance(model, self.MODEL):
            raise TypeError("%s trains a baselines.%s" % (type(self).__name__, self.MODEL.__name__))
        self.model = model
        self.opt = FusedAdam(model.parameters(), lr=lr, betas=betas)
        self.sync = ops.default_sync() if sync is None else sync
        self._one = None

    def _drop_inference_caches(self):
        for m in self._inference_caches():
            m._derived = None

    def _update(self, *batch):
        """One Adam update; (loss, accuracy) of the batch before it, as device scalars: nothing is read back here."""
        if ops.matrix_path() != "fp32":
            raise RuntimeError("%s runs on the fp32 matrix path only (ops.set_matrix_path('fp32')): the fp16 path and its "
                               "loss scale are not implemented for the baseline" % type(self).__name__)
        self.opt.zero_grad()
        loss, acc = self._loss_and_accuracy(*batch)
        if self._one is None or self._one.device != loss.device:
            self._one = torch.ones(1, device=loss.device, dtype=torch.float32)
        with ops.caller_thread_backward():
            loss.backward(self._one)
        self.opt.step()
        self._drop_inference_caches()
        return loss.detach().view(()), acc

    def state_dict(self):
        """{'model': the reference's state dict of the model (names, shapes, order; on the host), 'opt': torch.optim.Adam's format}."""
        return {"model": {k: v.detach().to("cpu").contiguous() for k, v in self.model.state_dict().items()}, "opt": self.opt.state_dict()}

    def load_state_dict(self, sd):
        self.model.load_state_dict(sd["model"], strict=True)
        if sd.get("opt") is not None:
            self.opt.load_state_dict(sd["opt"])
        self._drop_inference_caches()


class SiameseTrainer(_BaselineTrainer):
    """One FusedAdam over every parameter of a baselines.SiameseNet, in the reference's parameter order."""

    MODEL = SiameseNet

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), sync=None):
        super().__init__(model, lr, betas, sync)
        self.last_logits = None      # [B, 1] logits of the latest train_step (before its update), detached

    def _inference_caches(self):
        return self.model, self.model.embedding_net

    def _loss_and_accuracy(self, x1, x2, n_pos):
        logits = siamese_forward_train(self.model, x1, x2, self.sync)
        self.last_logits = logits.detach()
        return pair_loss(logits, n_pos), pair_accuracy(logits, n_pos)

    def train_step(self, x1, x2, n_pos):
        """One Adam update on the pair batch (x1[i], x2[i]); rows < n_pos are same-class pairs.  Returns (loss, accuracy) of the
        batch before the update, as device scalars: nothing is read back here.  Data-parallel: the rank's pairs (PairSampler.batch
        with rank and world), its own n_pos (0 .. all of them), its own mean loss and accuracy."""
        return self._update(x1, x2, n_pos)


def _rank_rows(batch_size, rank, world, who):
    """Rows [lo, hi) of a global batch that rank `rank` of `world` takes: equal shards (the BatchNorm merge and the mean of the
    ranks' mean losses rely on them)."""
    rank, world = int(rank), int(world)
    if world < 1 or not 0 <= rank < world:
        raise ValueError("%s: rank %d outside [0, world = %d)" % (who, rank, world))
    if batch_size % world:
        raise ValueError("%s: batch_size %d is not a multiple of world = %d" % (who, batch_size, world))
    per = batch_size // world
    return rank * per, (rank + 1) * per


class PairSampler:
    """Pair batches over a data.EpisodeBank: batch_size // 2 positive pairs (two DISTINCT images of one class) first, then negative
    pairs (one image each of two different classes).  Host logic only (a few dozen integers per batch); images are served by
    bank.gather, flips follow bank.mirror.  The draws of iteration `it` depend on (seed, it) alone: a resumed run sees the batches the
    uninterrupted run saw.  Reads bank.offsets and bank.mirror (and bank.gather in batch())."""

    def __init__(self, bank, batch_size, seed=0):
        self.bank = bank
        self.offsets = np.asarray(bank.offsets, dtype=np.int64)
        sizes = np.diff(self.offsets)
        self.classes = np.nonzero(sizes >= 1)[0]
        self.pos_classes = np.nonzero(sizes >= 2)[0]        # a class of one image is never drawn for a positive pair
        self.batch_size, self.n_pos, self.seed = int(batch_size), int(batch_size) // 2, int(seed)
        self.mirror = bool(bank.mirror)
        if self.batch_size < 1:
            raise ValueError("PairSampler: batch_size must be positive")
        if len(self.classes) < 2:
            raise ValueError("PairSampler: negative pairs need at least two classes, the bank has %d" % len(self.classes))
        if self.n_pos and not len(self.pos_classes):
            raise ValueError("PairSampler: positive pairs need a class with at least two images")

    def draw(self, it):
        """(idx [B, 2] int32 image indices, flip [B, 2] uint8, classes [B, 2]) of iteration `it`."""
        rng = np.random.default_rng([self.seed, 0x5A1A, int(it)])
        B = self.batch_size
        idx, cls = np.empty((B, 2), dtype=np.int32), np.empty((B, 2), dtype=np.int64)
        for b in range(B):
            if b < self.n_pos:
                c = int(self.pos_classes[rng.integers(len(self.pos_classes))])
                lo, hi = self.offsets[c], self.offsets[c + 1]
                idx[b] = lo + rng.choice(hi - lo, size=2, replace=False)
                cls[b] = c
            else:
                c2 = self.classes[rng.choice(len(self.classes), size=2, replace=False)]
                idx[b] = [self.offsets[c] + rng.integers(self.offsets[c + 1] - self.offsets[c]) for c in c2]
                cls[b] = c2
        flip = (rng.random((B, 2)) < 0.5) if self.mirror else np.zeros((B, 2), dtype=bool)
        return idx, flip.astype(np.uint8), cls

    def batch(self, it, rank=0, world=1):
        """(x1, x2, n_pos): the two halves of ONE gathered [2B, C, S, S] tensor.  world > 1: rows [rank * B / world,
        (rank + 1) * B / world) of the global draw of (seed, it); n_pos is then the number of those rows that are positive pairs
        (0, or all of them, for a rank on one side of the global n_pos)."""
        lo, hi = _rank_rows(self.batch_size, rank, world, "PairSampler")
        idx, flip, _ = self.draw(it)
        x = self.bank.gather(idx[lo:hi].T, flip[lo:hi].T)      # all first images, then all second images
        B = hi - lo
        return x[:B], x[B:], min(max(self.n_pos - lo, 0), B)


def _save(trainer, out_dir, step, model_key):
    ckpt_dir = os.path.join(out_dir, CHECKPOINT_DIR)
    os.makedirs(ckpt_dir, exist_ok=True)
    path = os.path.join(ckpt_dir, "model_%08d.pt" % step)
    tmp = path + ".tmp.%d" % os.getpid()
    sd = trainer.state_dict()
    torch.save({model_key: sd["model"], "opt": sd["opt"], "global_step": step}, tmp)
    os.replace(tmp, path)
    return path


def _train_loop(trainer, step_args, category, model_key, out_dir, args, n_iters, log_every, save_every, logger):
    """The loop of train_siamese and train_arcface: writes out_dir/args.json, resumes from the latest checkpoint of out_dir, runs
    trainer.train_step(*step_args(it)) up to iteration n_iters, logs (category, 'loss' / 'acc') every log_every iterations (one stacked
    host read per log point) and saves out_dir/ckpts/model_%08d.pt = {model_key, 'opt', 'global_step'} every save_every iterations and
    at the end.  Returns the trainer.
    Data-parallel (trainer.sync with world > 1; out_dir on a file system all ranks see): every rank resumes from the same checkpoint
    and runs the same iterations on its share of the batch (step_args(it, rank, world)); only rank 0 writes args.json, the checkpoints
    and the log, the others wait for a checkpoint to be complete; the logged loss and accuracy are the means over the ranks."""
    sync = trainer.sync if trainer.sync is not None and trainer.sync.world > 1 else None
    rank, world = (sync.rank, sync.world) if sync is not None else (0, 1)
    if rank == 0:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "args.json"), "w") as f:
            json.dump(args, f)
    step = 0
    ckpt_dir = os.path.join(out_dir, CHECKPOINT_DIR)
    has_ckpts = os.path.isdir(ckpt_dir)      # (every rank looks before any rank's first save: the same answer on all of them)
    if has_ckpts:
        try:
            latest = get_latest_ckpt(ckpt_dir)
        except FileNotFoundError:
            latest = None
        if latest is not None:
            sd = torch.load(latest, map_location="cpu", weights_only=False)
            trainer.load_state_dict({"model": sd[model_key], "opt": sd.get("opt")})
            step = int(sd["global_step"])
            print("Resuming {} training from iteration {}".format(category, step))
    if logger is None and rank == 0:
        logger = Logger(log_dir=os.path.join(out_dir, "logs"), img_dir=os.path.join(out_dir, "imgs"))
    if sync is not None:      # no rank writes a checkpoint while another still looks for the latest one
        _arrive(sync, trainer)

    def save():
        if rank == 0:
            _save(trainer, out_dir, step, model_key)
        if sync is not None:
            _arrive(sync, trainer)

    saved = step
    while step < n_iters:
        loss, acc = trainer.train_step(*(step_args(step) if sync is None else step_args(step, rank, world)))
        step += 1
        if log_every and step % log_every == 0:
            both = torch.stack([loss, acc])
            if sync is not None:
                both = sync.all_reduce_(both) / world
            loss_v, acc_v = both.tolist()
            if rank == 0:
                logger.add_scalar(category=category, k="loss", v=loss_v, global_step=step)
                logger.add_scalar(category=category, k="acc", v=acc_v, global_step=step)
        if save_every and step % save_every == 0:
            save()
            saved, has_ckpts = step, True
    if saved != step or not has_ckpts:
        save()
    return trainer


def _arrive(sync, trainer):
    """A barrier over what every sync has: an all-reduce whose result is read on the host."""
    dev = next(trainer.model.parameters()).device
    sync.all_reduce_(torch.zeros(1, device=dev, dtype=torch.float32)).tolist()


def train_siamese(device, bank, out_dir, n_iters, batch_size=128, lr=1e-3, log_every=100, save_every=1000, seed=0, logger=None):
    """Train a siamese baseline on the pair batches of `bank` up to iteration n_iters; resumes from the latest checkpoint of out_dir.
    Writes out_dir/args.json and out_dir/ckpts/model_%08d.pt = {'model', 'opt', 'global_step'} every save_every iterations and at
    the end; logs ('siamese', 'loss' / 'acc') every log_every iterations (one host read per log point).  Returns the trainer.
    Under torch.distributed with more than one rank (one process per GPU, every rank makes this same call): batch_size is the GLOBAL
    batch, a multiple of the world size; every rank builds the model from the same seed, see _train_loop for who writes what."""
    device = torch.device(device)
    args = {"baseline_type": "siamese", "img_size": int(bank.S), "img_channels": int(bank.C), "batch_size": int(batch_size),
            "lr": float(lr), "seed": int(seed), "n_iters": int(n_iters)}
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        net = ProtonetEmbeddingNet(inp_n_channels=bank.C, inp_img_size=bank.S)
        model = SiameseNet(net, net.embedding_dim)
    trainer = SiameseTrainer(model.to(device), lr=lr)
    sampler = PairSampler(bank, batch_size, seed)
    return _train_loop(trainer, sampler.batch, "siamese", "model", out_dir, args, n_iters, log_every, save_every, logger)


# ------------------------------------------------------------------------------------------------------
# ArcFace on the IR-SE backbone (baselines.ArcFace: arcface/models.py:62-84,120-164,170-229), training mode
# ------------------------------------------------------------------------------------------------------
ARC_S, ARC_M = 64.0, 0.5      # ArcfaceHead's scale and margin (arcface/models.py:172)


def _bn_train(x, bn, slope=None, sync=None):
    return ops.batch_norm(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.momentum, bn.eps, slope,
                          sync)


def dropout_offset(it, numel_local, rank=0, world=1):
    """Offset of a rank's first element in the dropout hash's counter at iteration `it`: iteration `it` owns the counters
    [it * N, (it + 1) * N) of the N = numel_local * world elements of the global batch, and rank r's rows are elements
    [r * numel_local, (r + 1) * numel_local) of it - the mask of a rank's rows is the mask those rows have in the whole batch."""
    return int(it) * (int(numel_local) * int(world)) + int(rank) * int(numel_local)


# Host switch (read once at import): GIM_NO_STRIDED_CONV=1 restores the stride-1 + subsample route of the stride-2 convolutions, for
# same-box A/B runs; the two routes differ by rounding only.
_STRIDED_CONV = os.environ.get("GIM_NO_STRIDED_CONV") is None


def irse_unit_train(unit, x, sync=None):
    """One bottleneck_IR_SE (a baselines._Unit) with batch statistics on an NHWC map.  The stride-2 3x3 convolution (padding 1) and the
    strided 1x1 shortcut convolution run as ops.conv2d_strided: forward, input gradient and weight gradient execute the convolution's
    own FLOPs.  (GIM_NO_STRIDED_CONV: at stride 1 through ops.conv2d - the stride-2 3x3 convolution as the even-position subsample of
    the stride-1 one, the shortcut as the 1x1 convolution of the subsampled input.)  The SE bottleneck's two 1x1 convolutions run on
    the [N, 1, 1, C] squeeze with the nn.Conv2d parameters themselves (their gradients land in the optimizer's bucket), the ReLU
    between them as ops.prelu without a slope.  sync: for the unit's BatchNorms (ops.batch_norm)."""
    r = unit.res_layer
    strided = unit.stride == 2 and _STRIDED_CONV
    h = ops.conv2d(_bn_train(x, r[0], None, sync), r[1].weight)
    h = ops.prelu(h, r[2].weight)
    if strided:
        h = ops.conv2d_strided(h, r[3].weight, stride=2)
    else:
        h = ops.conv2d(h, r[3].weight)
        if unit.stride == 2:
            h = ops.subsample2(h)
    h = _bn_train(h, r[4], None, sync)
    N, Ho, Wo, C = h.shape
    z = ops.mean_dim1(h.view(N, Ho * Wo, C)).view(N, 1, 1, C)
    gate = ops.conv2d(ops.prelu(ops.conv2d(z, r[5].fc1.weight), None), r[5].fc2.weight).view(N, C)
    if unit.cin == unit.depth:
        return ops.se_tail_train(h, gate, x, unit.stride)
    if strided:
        sc = ops.conv2d_strided(x, unit.shortcut_layer[0].weight, stride=2)
    else:
        sc = ops.conv2d(ops.subsample2(x) if unit.stride == 2 else x, unit.shortcut_layer[0].weight)
    return ops.se_tail_train(h, gate, _bn_train(sc, unit.shortcut_layer[1], None, sync), 1)


def arcface_forward_train(model, x, label, dropout=None, sync=None):
    """(emb [B, 512], logits [B, classes]) of a baselines.ArcFace as the reference's ``ArcFace.forward(x, label)`` gives them in
    training mode: batch statistics in every BatchNorm (running statistics updated), the margin head on the normalised embedding.
    dropout: (seed, it) - the mask of ``output_layer.1`` is a hash of (seed, it, element), nothing is stored; None: no dropout
    (required when the backbone's drop ratio is 0, an error otherwise).  Differentiable in every parameter; the model's ``training``
    flag is neither read nor changed.  label: int64 [B] on the device.
    sync (ops.DistSync): x and label are this rank's equal share of the batch (one image is enough when the ranks together have two);
    the BatchNorm statistics are over all ranks' images and the dropout mask is that of the rank's rows in the whole batch."""
    if not isinstance(model, ArcFace) or not isinstance(model.emb_model, Backbone):
        raise TypeError("arcface_forward_train runs a baselines.ArcFace on a baselines.Backbone")
    net = model.emb_model
    dims = (net.img_channels, net.img_size, net.img_size)
    x = ops._req(x, "x")
    if x.dim() != 4 or tuple(x.shape[1:]) != dims:
        raise RuntimeError("expected [B, %d, %d, %d] images, got %s" % (dims + (tuple(x.shape),)))
    B = x.shape[0]
    rank, world = (sync.rank, sync.world) if sync is not None else (0, 1)
    if B < 1 or B * world < 2:
        raise RuntimeError("batch statistics need at least two images")
    label = ops._req_label(label, B)
    p = float(net.output_layer[1].p)
    if p > 0.0 and dropout is None:
        raise RuntimeError("the backbone drops %.2f of output_layer.1: pass dropout=(seed, it)" % p)
    h = ops.conv2d(ops.to_nhwc(x), net.input_layer[0].weight)
    h = _bn_train(h, net.input_layer[1], net.input_layer[2].weight, sync)
    for unit in net.body:
        h = irse_unit_train(unit, h, sync)
    out = net.output_layer
    h = _bn_train(h, out[0], None, sync)
    if p > 0.0:
        seed, it = dropout
        h = ops.dropout(h, p, int(seed), dropout_offset(it, h.numel(), rank, world))
    e = ops.to_nchw(h).view(B, -1)      # the reference's (c, h, w) flatten order
    e = _bn_train(ops.linear(e, out[3].weight, out[3].bias), out[4], None, sync)
    emb = ops.l2norm_rows_train(e)
    cos = ops.BgemmFn.apply(emb[None], ops.col_l2norm(model.head.kernel)[None], 0, 0)[0]
    return emb, ops.arc_margin(cos, label, ARC_S, ARC_M)


def _row_mean(v):
    return ops.SumDim1Fn.apply(v.view(1, -1, 1), 1.0 / v.numel())


def margin_softmax_loss_and_accuracy(logits, label):
    """(mean cross-entropy of the margin logits, a differentiable [1] tensor; top-1 accuracy, a device scalar) from ONE pass over
    the logits: the cross-entropy kernel also writes whether each row's first largest logit is the label's."""
    per, correct = ops.softmax_ce(logits, label)
    return _row_mean(per).view(1), _row_mean(correct).view(())


def margin_softmax_loss(logits, label):
    """Mean cross-entropy of the margin logits over the batch: a [1] tensor."""
    return margin_softmax_loss_and_accuracy(logits, label)[0]


def top1_accuracy(logits, label):
    """Share of rows whose first largest logit is the label's; a device scalar."""
    return margin_softmax_loss_and_accuracy(logits.detach(), label)[1]


class ArcFaceTrainer(_BaselineTrainer):
    """One FusedAdam over every parameter of a baselines.ArcFace, in the reference's parameter order (head.kernel last).
    seed (>= 0): the dropout mask of output_layer.1 is a hash of (seed, iteration, element); train_arcface passes its own seed."""

    MODEL = ArcFace

    def __init__(self, model, lr=1e-4, betas=(0.9, 0.999), seed=0, sync=None):
        super().__init__(model, lr, betas, sync)
        if int(seed) < 0:
            raise ValueError("ArcFaceTrainer: seed must not be negative (it keys the dropout hash)")
        self.seed = int(seed)
        self.last_logits = None      # [B, classes] margin logits of the latest train_step (before its update), detached
        self.last_emb = None

    def _inference_caches(self):
        return (self.model.emb_model,)

    def _loss_and_accuracy(self, x, label, it):
        p = float(self.model.emb_model.output_layer[1].p)
        emb, logits = arcface_forward_train(self.model, x, label, (self.seed, it) if p > 0.0 else None, self.sync)
        self.last_logits, self.last_emb = logits.detach(), emb.detach()
        return margin_softmax_loss_and_accuracy(logits, label)

    def train_step(self, x, label, it):
        """One Adam update on the class-labelled batch (x, label); `it` keys the dropout mask.  Returns (loss, accuracy) of the batch
        before the update, as device scalars: nothing is read back here."""
        return self._update(x, label, it)


class IdentitySampler:
    """Class-labelled batches over a data.EpisodeBank, the ``ArcfaceDataSet.__getitem__`` contract (data_handling/img_datasets.py:
    217-270): the class uniform over the bank's (non-empty) classes, the image uniform within the class, a horizontal flip with
    probability 1/2 when bank.mirror.  Host logic only; the draws of iteration `it` depend on (seed, it) alone.  Labels are positions
    in the bank's class list (0 .. n_classes - 1).  Reads bank.offsets and bank.mirror (and bank.gather in batch())."""

    def __init__(self, bank, batch_size, seed=0):
        self.bank = bank
        self.offsets = np.asarray(bank.offsets, dtype=np.int64)
        self.sizes = np.diff(self.offsets)
        self.n_classes = len(self.sizes)
        self.classes = np.nonzero(self.sizes >= 1)[0]
        self.batch_size, self.seed = int(batch_size), int(seed)
        self.mirror = bool(bank.mirror)
        if self.batch_size < 2:
            raise ValueError("IdentitySampler: batch_size must be at least 2 (batch statistics)")
        if not len(self.classes):
            raise ValueError("IdentitySampler: the bank has no images")

    def draw(self, it):
        """(idx [B] int32 image indices, flip [B] uint8, label [B] int64) of iteration `it`."""
        rng = np.random.default_rng([self.seed, 0xA2CF, int(it)])
        B = self.batch_size
        label = self.classes[rng.integers(len(self.classes), size=B)].astype(np.int64)
        pos = rng.integers(self.sizes[label])      # one bound per row: uniform within the row's class
        idx = (self.offsets[label] + pos).astype(np.int32)
        flip = (rng.random(B) < 0.5) if self.mirror else np.zeros(B, dtype=bool)
        return idx, flip.astype(np.uint8), label

    def batch(self, it, rank=0, world=1):
        """(x [B, C, S, S], label int64 [B]) on the bank's device.  world > 1: rows [rank * B / world, (rank + 1) * B / world) of the
        global draw of (seed, it)."""
        lo, hi = _rank_rows(self.batch_size, rank, world, "IdentitySampler")
        idx, flip, label = self.draw(it)
        x = self.bank.gather(idx[lo:hi], flip[lo:hi])
        return x, torch.from_numpy(label[lo:hi]).to(x.device, non_blocking=True)


def train_arcface(device, bank, out_dir, n_iters, num_layers=50, batch_size=128, lr=1e-4, drop_ratio=0.6, th=1.5, log_every=100,
                  save_every=1000, seed=0, logger=None):
    """Train an ArcFace baseline (IR-SE backbone, 512-d embedding, one class per class of `bank`) on the class-labelled batches of
    `bank` up to iteration n_iters; resumes from the latest checkpoint of out_dir and then sees the batches and dropout masks the
    uninterrupted run saw.  Writes out_dir/args.json (what authentication_eval.get_arcface_authenticator reads: img_size,
    img_channels, num_layers, dropout, emb_dim, th) and out_dir/ckpts/model_%08d.pt = {'arcface', 'opt', 'global_step'} every
    save_every iterations and at the end; logs ('arcface', 'loss' / 'acc') every log_every iterations.  Returns the trainer.
    Under torch.distributed with more than one rank: as train_siamese (batch_size is the GLOBAL batch, a multiple of the world size).

    th is stored as given: the decision threshold of ArcFace.predict on the score -|e1 - e2|^2 <= 0.  The reference's default of 1.5
    can never be reached by such a score; calibrating it is a step of its own on held-out data,
    authentication_eval.calibrate_baseline(device, 'arcface', out_dir, ds, batch_size), which rewrites th in args.json."""
    device = torch.device(device)
    if num_layers not in (50, 100, 152):
        raise ValueError("train_arcface: num_layers should be 50, 100 or 152")
    if int(bank.S) not in (32, 64):
        raise ValueError("train_arcface: the backbone takes 32 x 32 or 64 x 64 images, the bank has %d" % int(bank.S))
    if not 0.0 <= drop_ratio < 1.0:
        raise ValueError("train_arcface: drop_ratio must be in [0, 1)")
    if int(batch_size) < 2:
        raise ValueError("train_arcface: batch_size must be at least 2 (batch statistics)")
    if n_iters < 0:
        raise ValueError("train_arcface: n_iters must not be negative")
    if int(seed) < 0:
        raise ValueError("train_arcface: seed must not be negative (it keys the sampler and the dropout hash)")
    n_classes = len(bank.offsets) - 1
    if n_classes < 2:
        raise ValueError("train_arcface: the margin softmax needs at least two classes, the bank has %d" % n_classes)
    args = {"baseline_type": "arcface", "img_size": int(bank.S), "img_channels": int(bank.C), "num_layers": int(num_layers),
            "dropout": float(drop_ratio), "emb_dim": 512, "th": float(th), "n_classes": n_classes, "batch_size": int(batch_size),
            "lr": float(lr), "seed": int(seed), "n_iters": int(n_iters)}
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        model = ArcFace(Backbone(num_layers, drop_ratio, 'ir_se', int(bank.S), int(bank.C)), 512, n_classes, th=th)
        with torch.no_grad():      # ArcfaceHead's initial kernel (arcface/models.py:177): uniform columns of unit norm
            model.head.kernel.uniform_(-1, 1).renorm_(2, 1, 1e-5).mul_(1e5)
    trainer = ArcFaceTrainer(model.to(device), lr=lr, seed=seed)
    sampler = IdentitySampler(bank, batch_size, seed)
    return _train_loop(trainer, lambda it, rank=0, world=1: sampler.batch(it, rank, world) + (it,), "arcface", "arcface", out_dir, args, n_iters, log_every, save_every,
                       logger)
