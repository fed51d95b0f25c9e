"""Baseline authenticators of the reference's authentication evaluation on the engine, inference only:
the siamese net (``baselines/siamese/models.py:14-56,97-114``) and ArcFace on the IR-SE backbone
(``baselines/arcface/models.py:16-164,214-237``), as ``eval_gim_on_authentication.py:47-72,109-128`` runs them
(``train(mode=False)`` + ``torch.no_grad()``).  Training the siamese net (batch statistics, its own forward over these modules'
parameters) is ``baseline_training.py``; the classes here keep raising in training mode.

The ``nn`` module tree exists for the ``state_dict`` only: names, shapes and order of its entries are the reference's, so
that a checkpoint written there loads with ``strict=True``.  No torch module ever computes: the forwards run on the
library's inference operators (``ops.conv2d_infer`` and friends, NHWC) over *derived* parameters that are computed once per
loaded state - in fp64 on the host, stored fp32 on the parameters' device, dropped by ``load_state_dict`` and ``.to()``:

* a BatchNorm BEHIND a convolution / linear is folded into it: ``w' = w * s[co]``, ``b' = b * s + t`` with
  ``s = gamma / sqrt(running_var + eps)``, ``t = beta - running_mean * s`` (exact);
* a BatchNorm IN FRONT of a zero-padded convolution stays a ``(s, t)`` pair: folded into the weights, its shift would
  have to appear in the padding as well.  It is applied by the ``se_tail`` of the unit in front (second output), the first
  one by the forward's only ``channel_affine``;
* a BatchNorm in front of flatten + linear (no padding) is folded into the linear's columns and bias;
* convolution weights are stored ``[Cout][KH][KW][Cin]``; the columns of the flatten-then-linear layers are permuted from
  the reference's ``(c, h, w)`` flatten order to the engine's ``(h, w, c)``.
"""
import torch
import torch.nn as nn

from . import ops

_BN_KEYS = ("weight", "bias", "running_mean", "running_var")


def bn_scale_shift(weight, bias, running_mean, running_var, eps):
    """(s, t) with batch_norm(x) = x * s + t in inference mode."""
    s = weight / torch.sqrt(running_var + eps)
    return s, bias - running_mean * s


def fold_bn_behind(w, b, s, t):
    """BatchNorm (s, t) behind a conv / linear with weight w [Cout, ...] and bias b (or None): the equivalent (w', b')."""
    wf = w * s.view(-1, *([1] * (w.dim() - 1)))
    return wf, (t if b is None else b * s + t)


def fold_bn_in_front_of_linear(w, b, s_cols, t_cols):
    """A per-column affine (s, t) in front of a linear [out, in]: W (x * s + t) + b = (W * s) x + (W t + b)."""
    return w * s_cols.view(1, -1), (w * t_cols.view(1, -1)).sum(1) + (0 if b is None else b)


def flatten_perm(C, H, W):
    """perm with  nhwc_flat[j] == nchw_flat[perm[j]]: column j of a linear that reads the (h, w, c)-flattened map is column
    perm[j] of the linear that reads the (c, h, w)-flattened one."""
    return torch.arange(C * H * W).view(C, H, W).permute(1, 2, 0).reshape(-1)


def conv_phys(w):
    """[Cout, Cin, KH, KW] -> the library's [Cout][KH][KW][Cin]."""
    return w.permute(0, 2, 3, 1).contiguous()


class _InferenceNet(nn.Module):
    """Derived-parameter cache: built on first use, dropped whenever the stored state may have changed."""

    def __init__(self):
        super().__init__()
        self._derived = None
        self.register_load_state_dict_post_hook(_drop_derived)

    def _apply(self, fn, *args, **kwargs):
        self._derived = None
        return super()._apply(fn, *args, **kwargs)

    def _state64(self):
        return {k: v.detach().to("cpu", torch.float64) for k, v in self.state_dict().items() if v.is_floating_point()}

    def _device(self):
        return next(self.parameters()).device

    def derived(self):
        if self._derived is None:
            dev = self._device()
            self._derived = _to_device(self._derive(self._state64()), dev)
        return self._derived

    def _enter(self, x, dims):
        if self.training:
            raise RuntimeError("batch statistics are not implemented: inference only (call .eval() / .train(mode=False))")
        x = ops._req(x, "x")
        if x.dim() != 4 or tuple(x.shape[1:]) != dims:
            raise RuntimeError("expected [N, %d, %d, %d] images, got %s" % (dims + (tuple(x.shape),)))
        if torch.is_grad_enabled() and x.requires_grad:
            raise RuntimeError("inference only: call under torch.no_grad()")
        with torch.no_grad():
            return ops.ToNHWCFn.apply(x)


def _drop_derived(module, incompatible_keys):
    module._derived = None


def _to_device(obj, dev):
    if torch.is_tensor(obj):
        return obj.to(dev, torch.float32).contiguous()
    if isinstance(obj, dict):
        return {k: _to_device(v, dev) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [_to_device(v, dev) for v in obj]
    return obj


def _bn(sd, prefix, eps):
    return bn_scale_shift(*(sd[prefix + k] for k in _BN_KEYS), eps)


# ------------------------------------------------------------------------------------------------------
# siamese
# ------------------------------------------------------------------------------------------------------
class ProtonetEmbeddingNet(_InferenceNet):
    """Four blocks conv3x3 -> BatchNorm -> ReLU -> MaxPool2d(2).  Each runs as one convolution with the BatchNorm folded in and
    one pool pass that applies the ReLU (it commutes with the maximum).  The embedding comes out flattened in (h, w, c) order;
    ``to_reference_order`` gives the reference's (c, h, w)."""

    def __init__(self, inp_n_channels, inp_img_size, hidden_dim=64, z_dim=64):
        super().__init__()
        self.inp_n_channels, self.inp_img_size, self.z_dim = inp_n_channels, inp_img_size, z_dim
        widths = [inp_n_channels, hidden_dim, hidden_dim, hidden_dim, z_dim]
        self.encoder = nn.Sequential(*[nn.Sequential(nn.Conv2d(a, b, 3, padding=1), nn.BatchNorm2d(b)) for a, b in zip(widths, widths[1:])])

    @property
    def out_img_size(self):
        return self.inp_img_size // 16

    @property
    def embedding_dim(self):
        return self.z_dim * self.out_img_size ** 2

    def _derive(self, sd):
        blocks = []
        for i, blk in enumerate(self.encoder):
            pre = "encoder.%d." % i
            w, b = fold_bn_behind(sd[pre + "0.weight"], sd[pre + "0.bias"], *_bn(sd, pre + "1.", blk[1].eps))
            blocks.append((conv_phys(w), b))
        return {"blocks": blocks}

    def forward(self, x):
        h = self._enter(x, (self.inp_n_channels, self.inp_img_size, self.inp_img_size))
        with torch.no_grad():
            for w, b in self.derived()["blocks"]:
                h = ops.maxpool2(ops.conv2d_infer(h, w, b), relu=True)
            return h.view(h.shape[0], -1)

    def to_reference_order(self, emb):
        s = self.out_img_size
        return emb.view(-1, s, s, self.z_dim).permute(0, 3, 1, 2).reshape(emb.shape[0], -1)


class SiameseNet(_InferenceNet):
    def __init__(self, embedding_net, embedding_dim):
        super().__init__()
        self.embedding_net = embedding_net
        self.fc = nn.Linear(embedding_dim, 1)

    def _derive(self, sd):
        net = self.embedding_net
        s = net.out_img_size
        return {"fc_w": sd["fc.weight"][:, flatten_perm(net.z_dim, s, s)], "fc_b": sd["fc.bias"]}

    def encode(self, x):
        return self.embedding_net(x)

    def classify(self, emb1, emb2):
        """Logits [B, 1] of two embeddings in the embedding net's (h, w, c) order."""
        if self.training:
            raise RuntimeError("batch statistics are not implemented: inference only (call .eval() / .train(mode=False))")
        emb1 = ops._req(emb1, "emb1")
        d = self.derived()
        with torch.no_grad():
            return ops.linear_infer(ops.absdiff(emb1, emb2), d["fc_w"], d["fc_b"])

    def forward(self, x1, x2):
        e = self.encode(torch.cat([x1, x2], 0))      # one pass over both inputs
        return self.classify(e[:x1.shape[0]], e[x1.shape[0]:])


# ------------------------------------------------------------------------------------------------------
# ArcFace IR-SE
# ------------------------------------------------------------------------------------------------------
_STAGE_UNITS = {50: (3, 4, 14, 3), 100: (3, 13, 30, 3), 152: (3, 8, 36, 3)}
_STAGE_DEPTH = (64, 128, 256, 512)


def unit_plan(num_layers):
    """[(in_channel, depth, stride)] of the body's units: each stage opens with a stride-2 unit."""
    plan, cin = [], 64
    for depth, n in zip(_STAGE_DEPTH, _STAGE_UNITS[num_layers]):
        plan += [(cin if j == 0 else depth, depth, 2 if j == 0 else 1) for j in range(n)]
        cin = depth
    return plan


class _SE(nn.Module):
    def __init__(self, channels, reduction):
        super().__init__()
        self.fc1 = nn.Conv2d(channels, channels // reduction, 1, bias=False)
        self.fc2 = nn.Conv2d(channels // reduction, channels, 1, bias=False)


class _Unit(nn.Module):
    """Parameter container of one bottleneck_IR_SE (keys shortcut_layer.{0,1}.*, res_layer.{0..5}.*)."""

    def __init__(self, cin, depth, stride):
        super().__init__()
        self.cin, self.depth, self.stride = cin, depth, stride
        if cin == depth:
            self.shortcut_layer = nn.Identity()       # MaxPool2d(1, stride): a subsample, done by se_tail
        else:
            self.shortcut_layer = nn.Sequential(nn.Conv2d(cin, depth, 1, stride, bias=False), nn.BatchNorm2d(depth))
        self.res_layer = nn.Sequential(nn.BatchNorm2d(cin), nn.Conv2d(cin, depth, 3, 1, 1, bias=False), nn.PReLU(depth),
                                       nn.Conv2d(depth, depth, 3, stride, 1, bias=False), nn.BatchNorm2d(depth), _SE(depth, 16))


def derive_unit(sd, pre, unit):
    """Derived parameters of one unit from an fp64 state dict (keys under `pre`)."""
    r = pre + "res_layer."
    d = {"bn_in": _bn(sd, r + "0.", unit.res_layer[0].eps), "w1": conv_phys(sd[r + "1.weight"]), "a1": sd[r + "2.weight"]}
    w2, b2 = fold_bn_behind(sd[r + "3.weight"], None, *_bn(sd, r + "4.", unit.res_layer[4].eps))
    d["w2"], d["b2"] = conv_phys(w2), b2
    d["fc1"], d["fc2"] = conv_phys(sd[r + "5.fc1.weight"]), conv_phys(sd[r + "5.fc2.weight"])
    d["relu"] = torch.zeros(d["fc1"].shape[0], dtype=torch.float64)
    if unit.cin != unit.depth:
        s = pre + "shortcut_layer."
        ws, bs = fold_bn_behind(sd[s + "0.weight"], None, *_bn(sd, s + "1.", unit.shortcut_layer[1].eps))
        d["ws"], d["bs"] = conv_phys(ws), bs
    return d


def run_unit(x, xb, d, stride, next_bn=None):
    """One IR-SE unit: x the raw input (shortcut path), xb its leading BatchNorm applied.  At most 7 launches: conv1 (+PReLU),
    conv2 (+folded BN), shortcut 1x1 (where the widths differ), squeeze, two SE linears, se_tail.  Returns out, or (out, next_bn(out))."""
    r = ops.conv2d_infer(xb, d["w1"], None, d["a1"])
    r = ops.conv2d_infer(r, d["w2"], d["b2"], None, stride)
    N, Ho, Wo, C = r.shape
    if "ws" in d:
        sc, ss = ops.conv2d_infer(x, d["ws"], d["bs"], None, stride), 1
    else:
        sc, ss = x, stride
    z = ops.mean_dim1(r.view(N, Ho * Wo, C))
    z = ops.conv2d_infer(z.view(N, 1, 1, C), d["fc1"], None, d["relu"])
    gate = ops.conv2d_infer(z, d["fc2"]).view(N, C)
    if next_bn is None:
        return ops.se_tail(r, gate, sc, ss)
    return ops.se_tail(r, gate, sc, ss, next_bn[0], next_bn[1])


class Backbone(_InferenceNet):
    def __init__(self, num_layers, drop_ratio, mode='ir', img_size=64, img_channels=3):
        super().__init__()
        if num_layers not in _STAGE_UNITS:
            raise ValueError("num_layers should be 50, 100 or 152")
        if mode == 'ir':
            raise NotImplementedError("mode='ir' is not used by the authentication evaluation: only 'ir_se' is implemented")
        if mode != 'ir_se':
            raise ValueError("mode should be ir or ir_se")
        if img_size not in (32, 64):
            raise ValueError("img_size should be 32 or 64")
        self.img_size, self.img_channels, self.last_img_size = img_size, img_channels, img_size // 16
        self.input_layer = nn.Sequential(nn.Conv2d(img_channels, 64, 3, 1, 1, bias=False), nn.BatchNorm2d(64), nn.PReLU(64))
        self.output_layer = nn.Sequential(nn.BatchNorm2d(512), nn.Dropout(drop_ratio), nn.Flatten(),
                                          nn.Linear(512 * self.last_img_size ** 2, 512), nn.BatchNorm1d(512))
        self.body = nn.Sequential(*[_Unit(*u) for u in unit_plan(num_layers)])

    def _derive(self, sd):
        w0, b0 = fold_bn_behind(sd["input_layer.0.weight"], None, *_bn(sd, "input_layer.1.", self.input_layer[1].eps))
        d = {"w0": conv_phys(w0), "b0": b0, "a0": sd["input_layer.2.weight"],
             "units": [derive_unit(sd, "body.%d." % i, u) for i, u in enumerate(self.body)]}
        # output layer: BatchNorm2d -> (dropout) -> flatten -> Linear -> BatchNorm1d, all folded into one linear over (h, w, c)
        s = self.last_img_size
        s2, t2 = _bn(sd, "output_layer.0.", self.output_layer[0].eps)
        w, b = fold_bn_in_front_of_linear(sd["output_layer.3.weight"], sd["output_layer.3.bias"],
                                          s2.repeat_interleave(s * s), t2.repeat_interleave(s * s))
        w, b = fold_bn_behind(w, b, *_bn(sd, "output_layer.4.", self.output_layer[4].eps))
        d["wo"], d["bo"] = w[:, flatten_perm(512, s, s)], b
        return d

    def embed_raw(self, x):
        """The 512-d embedding BEFORE l2 normalisation (ops.pair_score normalises)."""
        h = self._enter(x, (self.img_channels, self.img_size, self.img_size))
        d = self.derived()
        units = d["units"]
        with torch.no_grad():
            h = ops.conv2d_infer(h, d["w0"], d["b0"], d["a0"])
            hb = ops.channel_affine(h, *units[0]["bn_in"])
            for i, u in enumerate(self.body):
                if i + 1 < len(units):
                    h, hb = run_unit(h, hb, units[i], u.stride, units[i + 1]["bn_in"])
                else:
                    h = run_unit(h, hb, units[i], u.stride)
            return ops.linear_infer(h.view(h.shape[0], -1), d["wo"], d["bo"])

    def forward(self, x):
        e = self.embed_raw(x)
        with torch.no_grad():
            return ops.l2norm_rows(e)


class _Head(nn.Module):
    """head.kernel: the margin-softmax class matrix.  Loaded for state-dict compatibility, never used in inference."""

    def __init__(self, embedding_size, classnum):
        super().__init__()
        self.kernel = nn.Parameter(torch.zeros(embedding_size, classnum))


class ArcFace(nn.Module):
    def __init__(self, emb_model, embedding_size, n_classes, th=1.5):
        super().__init__()
        self.emb_model = emb_model
        self.head = _Head(embedding_size, n_classes)
        self.embedding_size, self.n_classes, self.th = embedding_size, n_classes, th

    def forward(self, x, label=None):
        if label is not None:
            raise NotImplementedError("the ArcFace head (margin loss) is training code: inference only")
        return self.emb_model(x)

    def predict(self, x1, x2):
        """(score, score >= th), score = -|e1 - e2|^2 of the normalised embeddings; ONE pass of the backbone over both inputs."""
        e = self.emb_model.embed_raw(torch.cat([x1, x2], 0))
        with torch.no_grad():
            score = ops.pair_score(e[:x1.shape[0]], e[x1.shape[0]:])
        return score, score.ge(self.th)
