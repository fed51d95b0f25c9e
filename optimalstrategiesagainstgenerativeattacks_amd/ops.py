"""Autograd operators over the C ABI of libgim_hip.so (include/gim_hip.h).

Every operator here launches hand-written HIP kernels on torch's current stream through ctypes;
torch supplies device memory, streams and the autograd tape only.  There is no CPU path: tensors
must be CUDA(HIP) float32.  Activations are NHWC.
"""
import collections
import ctypes
import math
import os
import struct
import warnings
import weakref

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib, optim
from ._lib import GimConvShape, GimGemmJob, GimWgradJob, check

LRELU_SLOPE = 0.2

# Higher-order mode.  The only second-order quantity of the training path is the R1 regulariser
# (training/utils.py:115-124): the gradient of the authenticator's output w.r.t. its INPUT IMAGES, differentiated
# once more w.r.t. the parameters.  Inside `input_grad_only()` a backward that runs with create_graph=True returns
# differentiable input gradients (each first-order backward is itself a Function whose adjoint reuses the same
# kernels) and no parameter gradients; create_graph outside that context is refused rather than silently wrong.
_HIGHER = {"input_grad_only": False}


class input_grad_only:
    def __enter__(self):
        self.prev = _HIGHER["input_grad_only"]
        _HIGHER["input_grad_only"] = True

    def __exit__(self, *exc):
        _HIGHER["input_grad_only"] = self.prev


def _second_order():
    """True when this backward is being recorded (create_graph=True)."""
    if not torch.is_grad_enabled():
        return False
    if not _HIGHER["input_grad_only"]:
        raise NotImplementedError("create_graph=True is supported for input gradients only: wrap the autograd.grad call in "
                                  "ops.input_grad_only() (training_utils.compute_grad2 does)")
    return True


# Executed-work accounting (bench.py, tools/): inside `count_flops()` every convolution / linear / batched-GEMM launch adds
# the multiply-adds its kernel EXECUTES (the pool / sub-pixel folds run (K+1)^2 taps at a quarter of the pixels, not the
# K^2 full-resolution taps of the unfused reference op) to a Counter keyed by (kind, shape).  Off (None) otherwise.
_FLOPS = None
_PHASES = None     # phase_timeline(): a list that gim_step's phase marks are appended to


class phase_timeline:
    """with ops.phase_timeline() as marks: gim_step(...)  ->  marks = [(name, event), ...]: one timing event per phase boundary of the
    overlapped training step, recorded on the stream the phase runs on (lane 0 = the caller's stream, lane 1 = the discriminator's).
    bench.py --phases turns them into the step's timeline; nothing is recorded outside the context."""

    def __enter__(self):
        global _PHASES
        self.prev = _PHASES
        _PHASES = []
        return _PHASES

    def __exit__(self, *a):
        global _PHASES
        _PHASES = self.prev


def mark_phase(name):
    if _PHASES is not None:
        ev = torch.cuda.Event(enable_timing=True)
        ev.record(torch.cuda.current_stream())
        _PHASES.append((name, ev))


class count_flops:
    """with ops.count_flops() as c: ...   ->  c[(kind, cfg)] = [launches, executed FLOPs per launch]; kinds fwd / dgrad / wgrad / bgemm;
    cfg = (N, H, W, Cin, Cout, KH, ups, pool, fold) for convolutions and linears (H = W = KH = 1), (batch, M, N, K) for bgemm;
    pool = 2: the forward / wgrad launches of a pooled 3x3 conv on the box-filtered input (9 taps; its dgrad counts under pool = 1)."""

    def __enter__(self):
        global _FLOPS
        self.prev = _FLOPS
        _FLOPS = {}
        return _FLOPS

    def __exit__(self, *exc):
        global _FLOPS
        _FLOPS = self.prev


def conv_executed_flops(N, H, W, Cin, Cout, KH, ups, pool, fold):
    """2 * MACs one forward (= one dgrad = one wgrad) launch of this convolution executes.  (H, W) is the resolution the
    unfused conv would run at (after the nearest upsample, before the average pool)."""
    if pool == 2:            # ONE stride-2 conv with the conv's own K^2 taps on the box-filtered input (_pool_route "box")
        return 2.0 * N * (H >> 1) * (W >> 1) * Cin * Cout * KH * KH
    if fold and pool:        # ONE stride-2 conv, (K+1)^2 taps, on the pooled grid
        return 2.0 * N * (H >> 1) * (W >> 1) * Cin * Cout * (KH + 1) ** 2
    if fold and ups:         # 4 parity classes on the low-resolution grid, ((K+1)/2)^2 taps each
        return 2.0 * N * H * W * Cin * Cout * ((KH + 1) // 2) ** 2
    return 2.0 * N * H * W * Cin * Cout * KH * KH


def conv_algorithmic_flops(N, H, W, Cin, Cout, KH, *_):
    """2 * MACs of the unfused reference op (F.conv2d at the full resolution): the SURVEY.md 8(d) convention."""
    return 2.0 * N * H * W * Cin * Cout * KH * KH


def _note_conv(kind, geom, sh=None, plan_kind=None):
    """Count one conv launch (ops.count_flops).  sh / plan_kind (the launch's gim_conv_shape and its gim_conv_launch_plan kind): the
    library is asked which share of the launch's K steps its kernel skips (position-major rows on small maps skip padding taps) -
    skipped multiply-adds are not executed FLOPs."""
    ent = _FLOPS.get((kind, geom.key))
    if ent is None:
        share = 1.0 if sh is None else 1.0 - _launch_plan(sh, plan_kind, geom.key).skipped_permille / 1000.0
        _FLOPS[(kind, geom.key)] = [1, conv_executed_flops(*geom.key) * share]
    else:
        ent[0] += 1


def _note_bgemm(batch, M, N, K, launches=1):     # count `launches` batched-GEMM launches of one shape (ops.count_flops)
    if _FLOPS is not None:
        _FLOPS.setdefault(("bgemm", (batch, M, N, K)), [0, 2.0 * batch * M * N * K])[0] += launches


def _stream():
    """Raw handle of the caller's current HIP stream.  (torch.cuda.current_stream() builds a Stream object through several
    layers of Python, ~4 us; with ~1400 kernel calls per step that was 6 ms of the ~35 ms the host needs per step.)"""
    return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())


def _p(t, off=0):
    if t is None:
        return None
    return t.data_ptr() + 4 * off


def _req(t, name):
    if not (t.is_cuda and t.dtype == torch.float32):
        raise RuntimeError("%s must be a CUDA float32 tensor (got %s on %s): the GIM engine has no CPU path"
                           % (name, t.dtype, t.device))
    return t if t.is_contiguous() else t.contiguous()


def weight_phys(w):
    """The [Cout][KH][KW][Cin] storage view of a conv weight parameter (logical [Cout,Cin,KH,KW] kept
    channels-last), or the [out][in] linear weight itself.  The view is kept on the tensor object (keyed by its data pointer: a
    view follows in-place updates, only a re-allocated storage invalidates it) - building it costs 3 us, ~520 times per step."""
    try:
        c = w._gim_phys
        if c[0] == w.data_ptr():
            return c[1]
    except AttributeError:
        pass
    if w.dim() == 2:
        return w if w.is_contiguous() else w.contiguous()
    wp = w.permute(0, 2, 3, 1)
    if not wp.is_contiguous():
        return wp.contiguous()      # a copy: not cached (it would not follow updates of w)
    w._gim_phys = (w.data_ptr(), wp)
    return wp


# Deterministic weight-gradient combine (slabs + fixed-order reduce) instead of float atomics, for the non-queued path
_WGRAD_SLABS = os.environ.get("GIM_WGRAD_SLABS") is not None

# Deterministic mode (host switch GIM_DETERMINISTIC=1 at import, or set_deterministic()): the reference's path is reproducible
# from run to run (torch on the CPU, training/gim_img_training.py:157-183); the engine's default is not in its last bits, because
# three of its sums are combined with float atomics whose order varies: the K slices of forward / dgrad launches that split K,
# the pixel slices of a weight gradient (and the jobs of one gradient in the batched finish), the grouped style projections'
# input gradient.  Under the switch no launch splits K (tune_ksplit = 1 on every forward / dgrad shape), weight gradients go the
# non-queued way as slabs added in a fixed order (the GIM_WGRAD_SLABS path), and the style projections run one by one (autograd
# adds their gradients in graph order): two runs of one program are bit-identical, at ~25 % of the speed of the default
# (tests/test_gpu_models.py::test_deterministic_mode_is_bit_reproducible).
_DETERMINISTIC = [os.environ.get("GIM_DETERMINISTIC") is not None]


def deterministic():
    return _DETERMINISTIC[0]


def set_deterministic(flag):
    """Switch the deterministic mode (see above) on or off; returns the previous setting."""
    prev = _DETERMINISTIC[0]
    _DETERMINISTIC[0] = bool(flag)
    if prev != _DETERMINISTIC[0]:
        _SPLITS_K.clear()    # the cached "does this launch split K" answers were given for the other mode
    return prev


# Matrix path of the convolutions: "fp32" (default: fp32 operands on the fp32 MFMA - the reference's arithmetic, what every parity
# bound of north_star is stated for) or "fp16" (opt-in, BASELINE config 5 "fp16 MFMA"): operands rounded to fp16 when they are
# staged into LDS, v_mfma_f32_32x32x16_f16 with fp32 accumulation, fp32 master weights and fp32 activations in HBM
# (csrc/conv_f16.inc).  Host switch GIM_MATRIX_PATH=fp16 at import, or set_matrix_path(); launches that are not eligible (image
# layers with 1 / 3 / 6 channels, < 32 output channels, linears) stay on the fp32 MFMA.
_PREC = [1 if os.environ.get("GIM_MATRIX_PATH", "fp32") == "fp16" else 0]


def matrix_path():
    return "fp16" if _PREC[0] else "fp32"


# Loss scale of the fp16 matrix path.  Gradients of a mean-over-episodes loss reach the convolutions at 1e-3 ... 1e-7 per element;
# fp16 keeps 11 significant bits only down to 6.1e-5 (below that: subnormals, then zero).  The step functions (gim_img_training)
# therefore differentiate loss * S and the fused Adam kernel multiplies the gradient bucket by 1 / S (a power of two: exact in
# fp32, every backward operator is linear in the incoming gradient) - the standard mixed-precision recipe; not in the reference,
# which has no 16-bit path.  Too-large values saturate at +-65504 when they are rounded (conv_f16.inc).  1 on the fp32 path.
#
# GIM_FP16_LOSS_SCALE=dynamic / set_loss_scale("dynamic"): the scale lives in device memory, one optim.LossScaler per optimizer.
# The backward pass of a step function then runs its fp16 launches with the IEEE conversion (gim_conv_shape.prec = 2: a value
# beyond the fp16 range becomes an infinity instead of +-65504), the optimizer step looks for a non-finite value in its gradient
# bucket, skips the update when it finds one and halves the scale; growth_interval clean steps in a row double it
# (gim_adam_step_scaled; nothing of this is read back by the host).  Forward passes keep the saturating kernels: their values are
# not scaled, so no scale can bring them back into range.
_DYNAMIC_DEFAULTS = dict(init=4096.0, growth_interval=2000, min_scale=1.0)   # init: the static default; interval: torch.amp.GradScaler's
_warned_scales = set()


def _parse_loss_scale(value, what):
    """-> "dynamic" or a positive float; ValueError for anything else, one warning per value that is not a power of two (the
    "1 / S is exact" argument above needs one)."""
    if isinstance(value, str) and value.strip().lower() == "dynamic":
        return "dynamic"
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError("%s: %r is neither a number nor 'dynamic'" % (what, value)) from None
    if not (v > 0.0) or v == float("inf"):   # (also NaN)
        raise ValueError("%s must be a positive finite number or 'dynamic', got %r" % (what, value))
    if math.frexp(v)[0] != 0.5 and v not in _warned_scales:
        _warned_scales.add(v)
        warnings.warn("%s = %r is not a power of two: scaling and un-scaling the gradients then rounds" % (what, value), stacklevel=3)
    return v


_LOSS_SCALE = [_parse_loss_scale(os.environ.get("GIM_FP16_LOSS_SCALE", "4096"), "GIM_FP16_LOSS_SCALE")]
_DYNAMIC = dict(_DYNAMIC_DEFAULTS)   # what new optim.LossScaler objects start from in dynamic mode
_ARMED = [0]                         # inside the backward pass of a step function in dynamic mode: fp16 launches take prec 2


def loss_scale_mode():
    """"dynamic" (GIM_FP16_LOSS_SCALE=dynamic / set_loss_scale("dynamic"); in force on the fp16 matrix path only) or "static"."""
    return "dynamic" if _LOSS_SCALE[0] == "dynamic" else "static"


def loss_scale():
    """The static loss scale: 1 on the fp32 path; in dynamic mode the scalers' INITIAL scale (the current one lives on the device:
    optim.LossScaler.state())."""
    if not _PREC[0]:
        return 1.0
    return _DYNAMIC["init"] if _LOSS_SCALE[0] == "dynamic" else _LOSS_SCALE[0]


def dynamic_loss_scale_defaults():
    return dict(_DYNAMIC)


def set_loss_scale(value, init=4096, growth_interval=2000, min_scale=1.0):
    """A number (static scale) or "dynamic" (then init / growth_interval / min_scale are what new optim.LossScaler objects start
    from); returns the previous setting (a number or "dynamic")."""
    v = _parse_loss_scale(value, "loss scale")
    if v == "dynamic":
        i0, m0 = _parse_loss_scale(init, "init"), _parse_loss_scale(min_scale, "min_scale")
        if i0 == "dynamic" or m0 == "dynamic" or int(growth_interval) < 1:
            raise ValueError("dynamic loss scale: init and min_scale are positive numbers, growth_interval >= 1")
        _DYNAMIC.update(init=i0, growth_interval=int(growth_interval), min_scale=m0)
    prev = _LOSS_SCALE[0]
    _LOSS_SCALE[0] = v
    return prev


class armed_backward:
    """Context of a backward pass whose gradients a dynamic LossScaler will test: eligible fp16 launches inside (the second-order ones
    of the R1 term too) convert without the clamp.  A no-op for scaler None."""

    def __init__(self, scaler):
        self.on = 1 if scaler is not None else 0

    def __enter__(self):
        _ARMED[0] += self.on

    def __exit__(self, *exc):
        _ARMED[0] -= self.on


def set_matrix_path(name):
    """"fp32" or "fp16" (see above); returns the previous setting."""
    if name not in ("fp32", "fp16"):
        raise ValueError("matrix path must be 'fp32' or 'fp16'")
    prev = matrix_path()
    _PREC[0] = 1 if name == "fp16" else 0
    if prev != name:
        _SPLITS_K.clear()    # the cached launch plans were made for the other kernels
    return prev


_SHAPES = {}   # argument tuple -> template struct (a 17-field ctypes constructor costs 1.3 us, a copy of a template 0.4; ~640 per step)


def _shape(N, H, W, Cin, Cout, KH, ups, pre_slope, pool=0, wfold=0, res_ups=0):
    prec = 2 if (_PREC[0] and _ARMED[0]) else _PREC[0]
    key = (N, H, W, Cin, Cout, KH, ups, pre_slope, pool, wfold, res_ups, _DETERMINISTIC[0], prec)
    t = _SHAPES.get(key)
    if t is None:
        t = _SHAPES[key] = GimConvShape(N, H, W, Cin, Cout, KH, ups, pre_slope, pool, wfold, res_ups, 0, 1 if _DETERMINISTIC[0] else 0, 0, 0, 0.0,
                                        prec if H * W > 1 else 0)   # (linears - 1 x 1 maps - stay fp32: tiny, and the head's logits are built there)
    return GimConvShape.from_buffer_copy(t)    # callers set tune_* / post_slope / out_zeroed on their own copy


# Launch overrides for tools/step_autotune.py (tuning the launch table against the time of the WHOLE overlapped step instead of
# each kernel alone): {(kind, (N, H, W, Cin, Cout, KH, ups, pool, fold)): (tune_tile, tune_ksplit | tune_wgrad)} with kind
# "fwd" / "dgrad" / "wgrad".  Empty in the product: the compiled-in table and the heuristics decide.
_TUNE_OVERRIDE = {}


def _tuned(sh, kind, key):
    ov = _TUNE_OVERRIDE.get((kind, key)) if _TUNE_OVERRIDE else None
    if ov is not None:
        sh.tune_tile = ov[0]
        if kind == "wgrad":
            sh.tune_wgrad = ov[1]
        else:
            sh.tune_ksplit = ov[1]
    return sh


# Outputs of split-K launches.  A layer whose output tiles do not fill the chip is sliced along K over the grid and its slices
# are combined with float atomics into a ZEROED output: ~250 such launches per training step, each with its own memset in front
# (a 7 us fill kernel plus a kernel boundary).  Instead those outputs are carved out of pages that ONE torch.zeros call clears
# (per stream, 64 MB at a time): views keep their page alive, so tensor lifetimes are the usual ones; whether a launch splits K
# is asked from the library once per shape (gim_conv_launch_plan) and cached.
_ZERO_POOL = os.environ.get("GIM_NO_ZERO_POOL") is None   # A/B switch (host side)
_SPLITS_K = {}    # (plan kind,) + ConvGeom.key -> _Plan; cleared when the mode / matrix path / launch overrides change
_ZERO_PAGES = {}
_ZERO_PAGE = 16 << 20   # floats per page (64 MB)
_Plan = collections.namedtuple("_Plan", "ksplit skipped_permille")


def _launch_plan(sh, plan_kind, key):
    """What the library would launch for `sh` (include/gim_hip.h gim_conv_launch_plan; plan_kind 0 fwd, 1 dgrad, 2 dgrad_t), asked
    once per shape: the K-split factor (> 1: slices combined with atomics into a ZEROED output) and the skipped share of its K steps in 1/1000."""
    k_ = (plan_kind,) + key
    v = _SPLITS_K.get(k_)
    if v is None:
        out = (ctypes.c_int32 * 8)()
        check(_lib.load().gim_conv_launch_plan(ctypes.byref(sh), plan_kind, ctypes.cast(out, ctypes.c_void_p)), "conv_launch_plan")
        v = _SPLITS_K[k_] = _Plan(out[3], out[7] >> 8)
    return v


def _zeros_from_pool(shape, device):
    """A zero-filled float32 tensor of `shape`, cleared together with its neighbours by one fill per 64 MB page (pages are per
    (device, stream): the fill and the kernels that use the page are in stream order).  A view keeps its WHOLE page alive: outputs
    that live for one training step (saved activations) cost nothing extra, a tensor a caller keeps for long pins 64 MB - clone it."""
    n = 1
    for d in shape:
        n *= d
    na = (n + 63) & ~63
    if na > _ZERO_PAGE >> 1:     # a big output: its own fill (a view pins its whole page for as long as it lives)
        return torch.zeros(shape, device=device, dtype=torch.float32)
    raw = (torch._C._cuda_getDevice(), _stream())
    pg = _ZERO_PAGES.get(raw)
    if pg is None or pg[1] + na > pg[0].numel():
        pg = _ZERO_PAGES[raw] = [torch.zeros(_ZERO_PAGE, device=device, dtype=torch.float32), 0]
    v = pg[0][pg[1]:pg[1] + n].view(shape)
    pg[1] += na
    return v


def _conv_out(sh, plan_kind, key, shape, device):
    """Output buffer of a forward (plan_kind 0) / dgrad (1, 2) launch: zeros from the pool when the launch splits K (and
    sh.out_zeroed tells the library not to clear it again), plain torch.empty otherwise."""
    if _ZERO_POOL and _launch_plan(sh, plan_kind, key).ksplit > 1 and not torch.cuda.is_current_stream_capturing():
        sh.out_zeroed = 1
        return _zeros_from_pool(shape, device)
    return torch.empty(shape, device=device, dtype=torch.float32)


# --------------------------------------------------------------------------------------------
# spectral norm power iteration (no autograd: u, v are constants for the gradient, see ConvFn.backward)
# --------------------------------------------------------------------------------------------
@torch.no_grad()
def spectral_sigma(w, u, v, training):
    """torch.nn.utils.spectral_norm semantics; returns (sigma[1], u_used[Cout], v_used[K])."""
    lib = _lib.load()
    wp = weight_phys(w)
    Cout, Cin = w.shape[0], w.shape[1]
    KH = w.shape[2] if w.dim() == 4 else 1
    K = Cin * KH * KH
    sigma = torch.empty(1, device=w.device, dtype=torch.float32)
    u_s = torch.empty_like(u)
    v_s = torch.empty_like(v)
    scratch = torch.empty(9 * K + Cout, device=w.device, dtype=torch.float32)
    check(lib.gim_spectral_sigma(_p(wp), _p(u), _p(v), _p(sigma), _p(u_s), _p(v_s), _p(scratch), Cout, Cin, KH,
                                 1 if training else 0, _stream()), "spectral_sigma")
    return sigma, u_s, v_s


def _folded(wp, Cout, Cin, KH):
    """(KH+1)^2-tap folded weights F (sum of the 2x2-shifted copies of W) for the pool / sub-pixel forms."""
    f = torch.empty(Cout * (KH + 1) * (KH + 1) * Cin, device=wp.device, dtype=torch.float32)
    check(_lib.load().gim_conv2d_fold_weights(_p(wp), _p(f), Cout, Cin, KH, _stream()), "fold_weights")
    return f


class _StreamReady:
    """A buffer that ONE stream writes and others then use (the lanes and the encoders' side streams share WgradQueue pages, the job
    tables of the grouped launches and the weight copies of _WT_CACHE).  Built right after the writing work was issued on the current stream."""
    __slots__ = ("tensor", "event", "streams", "in_capture")

    def __init__(self, tensor):
        self.tensor = tensor
        self.rewritten()

    def rewritten(self):
        """The current stream has just (re)written the buffer: every other stream has to order itself behind that again."""
        self.event = torch.cuda.current_stream().record_event()
        self.streams = {_stream()}     # raw handles of the streams already ordered behind `event`
        self.in_capture = torch.cuda.is_current_stream_capturing()

    def use_on_current_stream(self, raw=None):
        """The buffer, safe to use in work issued on the current stream from now on (raw: its handle, when the caller has it).
        The first use on a stream other than the writer's makes that stream wait for the writer's event and tells the caching
        allocator about the second user; later uses are one set lookup on the raw handle - no torch Stream object is built.
        Capture rule: an event recorded BEFORE a hipGraph capture began is not waited for inside the capture.  That work has
        completed (a capture starts behind a device synchronisation, tools/graph_replay_experiment.py), and a captured wait on an
        un-captured event is not a graph edge.  An event recorded inside the capture is waited for: that is the edge."""
        if raw is None:
            raw = _stream()
        if raw not in self.streams:
            cur = torch.cuda.current_stream()
            if self.in_capture or not torch.cuda.is_current_stream_capturing():
                cur.wait_event(self.event)
            self.tensor.record_stream(cur)
            self.streams.add(raw)
        return self.tensor


# --------------------------------------------------------------------------------------------
# job tables of the grouped launches (one launch serves many layers and reads their jobs from device memory)
# --------------------------------------------------------------------------------------------
def layout_tables(jobs, *tables):
    """(bytes, offsets): a ctypes array of job structs (_lib.Gim*Job) and any number of int32 tables (lists of equal-length int
    tuples: which block works on what) as ONE buffer, every section at a multiple of 16 bytes.  An empty table becomes one
    placeholder row of two zeros, so that its launch is always handed a valid pointer."""
    blob, offsets = bytearray(), []
    for sec in [bytes(jobs)] + [struct.pack("<%di" % (len(t) * len(t[0])), *(v for row in t for v in row)) if t else bytes(8)
                                for t in tables]:
        blob += bytes(-len(blob) % 16)
        offsets.append(len(blob))
        blob += sec
    return bytes(blob), offsets


class _DeviceTable(_StreamReady):
    """layout_tables(...) in device memory: one pinned staging buffer (kept alive here: the copy is asynchronous), one copy on
    the current stream.  ptrs: device address of each section; extra: what the site keeps beside them (row counts, buffers the jobs
    point to).  Every launch first calls use_on_current_stream(raw): a stream other than the builder's then waits for the copy."""
    __slots__ = ("host", "ptrs", "extra")

    def __init__(self, jobs, *tables, extra=None):
        blob, offsets = layout_tables(jobs, *tables)
        self.host = torch.frombuffer(bytearray(blob), dtype=torch.uint8).pin_memory()
        super().__init__(self.host.to(torch.device("cuda", torch._C._cuda_getDevice()), non_blocking=True))
        self.ptrs, self.extra = [self.tensor.data_ptr() + o for o in offsets], extra


class _TableCache(collections.OrderedDict):
    """signature -> what build() made of it (a _DeviceTable), least recently used entry dropped beyond `capacity` (None: never).
    The signatures are addresses of parameters, their .grad buffers and allocator blocks, which repeat from step to step.  A miss
    inside a hipGraph capture cannot upload a table: get() raises or, with skip_in_capture, returns None."""

    def __init__(self, what, capacity=None, skip_in_capture=False):
        super().__init__()
        self.what, self.capacity, self.skip_in_capture = what, capacity, skip_in_capture

    def get(self, sig, build):
        if sig in self:
            self.move_to_end(sig)
        elif not (torch.cuda.is_initialized() and torch.cuda.is_current_stream_capturing()):
            self[sig] = build()
            if self.capacity is not None and len(self) > self.capacity:
                self.popitem(last=False)
        elif self.skip_in_capture:
            return None
        else:
            raise RuntimeError("%s: a job table not seen before; run eager warm-up steps (at least 2) before capturing a hipGraph" % self.what)
        return self[sig]


# --------------------------------------------------------------------------------------------
# deferred, batched weight-gradient finish
# --------------------------------------------------------------------------------------------
class _ArenaPage(_StreamReady):
    """One zero-filled page of a WgradQueue arena; its first `used` floats are handed out."""
    __slots__ = ("used",)

    def __init__(self, n, device):
        super().__init__(torch.zeros(n, device=device, dtype=torch.float32))
        self.used = 0

    def rezero(self):
        self.tensor[:self.used].zero_()
        self.used = 0
        self.rewritten()


class WgradQueue:
    """Weight gradients whose destination is the optimizer's flat gradient bucket are not finished one conv at a time
    (zero a slab, reduce it, un-fold it, spectral-norm chain rule, add: ~5 tiny launches per conv, ~900 per step).
    ConvFn.backward accumulates the raw gradient into a slot of a pre-zeroed arena and records a job; when the backward
    pass ends (autograd final callback) ALL jobs are finished by two launches (gim_wgrad_finish_batched) and the arena is
    cleared by one memset.  `.grad` is complete when backward() returns, exactly as before."""
    CHUNK = 4096
    PAGE = 32 << 20  # floats

    def __init__(self):
        self.pages = []       # _ArenaPage
        self.jobs = []        # tuples of ints (the job table signature)
        self.keep = []        # tensors that must outlive the flush
        self.streams = set()
        self.stream_of = {}   # raw stream handle -> torch Stream object
        self.cb_queued = False
        self.cache = _TableCache("WgradQueue", 16)   # job tuples -> _DeviceTable (G / D backward, buffer parities)
        self.enabled = os.environ.get("GIM_WGRAD_IMMEDIATE") is None

    def take(self, n, device):
        """n zeroed floats (64-float aligned) that stay valid until the flush."""
        n = (n + 63) & ~63
        if not self.pages or self.pages[-1].used + n > self.pages[-1].tensor.numel():
            # the zero-fill runs on the allocating stream; every OTHER stream that later adds into this page first waits for it
            self.pages.append(_ArenaPage(max(n, self.PAGE), device))
        pg = self.pages[-1]
        ptr = pg.use_on_current_stream().data_ptr() + 4 * pg.used
        pg.used += n
        return ptr

    def add(self, job, keep):
        self.jobs.append(job)
        self.keep.append(keep)
        raw = _stream()
        if raw not in self.stream_of:
            self.stream_of[raw] = torch.cuda.current_stream()
        self.streams.add(self.stream_of[raw])
        if not self.cb_queued:
            torch.autograd.Variable._execution_engine.queue_callback(self.flush)
            self.cb_queued = True

    def flush(self):
        self.cb_queued = False
        if not self.jobs:
            return
        cur = torch.cuda.current_stream()
        for st in self.streams:   # slots were written on the encoders' side streams too
            stream_wait(cur, st)
        sig = tuple(self.jobs)

        def build():
            arr = (GimWgradJob * len(sig))()
            tab, tab_sn = [], []
            targets = collections.Counter(jb[8] for jb in sig)   # grad_w pointers: a conv called several times in the pass has several jobs
            for j, jb in enumerate(sig):
                arr[j] = jb + (1 if targets[jb[8]] == 1 else 0,)    # exclusive
                blocks = [(j, c) for c in range(jb[14])]
                tab += blocks
                if jb[3]:
                    tab_sn += blocks
            return _DeviceTable(arr, tab, tab_sn, extra=(len(tab), len(tab_sn)))
        ent = self.cache.get(sig, build)
        raw = _stream()
        ent.use_on_current_stream(raw)
        (dj, dt, dsn), (nb, nbs) = ent.ptrs, ent.extra
        check(_lib.load().gim_wgrad_finish_batched(dj, len(sig), dt, nb, dsn, nbs, raw), "wgrad_finish_batched")
        if len(self.pages) > 1:  # first backward of a new shape: merge into one page for the next pass
            total = sum(pg.used for pg in self.pages)
            self.pages = [_ArenaPage(total + (total >> 3), self.pages[0].tensor.device)]
            self.cache.clear()
        else:
            # the re-zeroing runs on the flushing stream; the next pass's first user on every other stream waits for it
            self.pages[0].rezero()
        self.jobs, self.keep, self.streams = [], [], set()


# Lanes: the generator step's backward and the discriminator step overlap on the GPU (gim_img_training.gim_step);
# each lane has its own arena / job queue (and its own side streams, gim_img_models._side_streams).
_LANE = [0]
_QUEUES = {0: WgradQueue()}
wgrad_queue = _QUEUES[0]


def reset_wgrad_queues():
    """Drop weight-gradient jobs that a failed backward pass (exception inside autograd) left behind, re-zero their arena
    slots and re-arm the end-of-backward callback.  Called by FusedAdam.zero_grad(): a new iteration never inherits them."""
    for q in _QUEUES.values():
        if q.jobs or q.cb_queued:
            for pg in q.pages:
                if pg.used:
                    pg.rezero()
            q.jobs, q.keep, q.streams, q.cb_queued = [], [], set(), False


def current_lane():
    return _LANE[0]


def _queue():
    q = _QUEUES.get(_LANE[0])
    if q is None:
        q = _QUEUES[_LANE[0]] = WgradQueue()
    return q


def stream_wait(waiter, other):
    """waiter.wait_stream(other), skipped when both are the same HIP stream.  The role -> stream map of gim_img_models aliases
    roles onto shared streams (lane 1's first encoder runs on lane 1's own stream): a stream "waiting for itself" is a no-op in
    eager execution, but inside a hipGraph capture it records an event on the capturing stream and then makes that same stream
    wait for it - a self-edge in the captured graph (tools/graph_replay_experiment.py captures the two-lane step)."""
    if waiter.cuda_stream != other.cuda_stream:
        waiter.wait_stream(other)


# Backward's Python on the CALLING thread.  torch's autograd engine hands a backward pass to a per-device worker thread; every node
# of this engine is a Python Function, and with the hand-off the host needs 31-37 ms to enqueue one training step where it needs 26-28 ms
# when the calling thread runs the nodes itself (64x64x3, 16 episodes: the device needs 37 ms, so with the worker thread the host IS the
# bound in part of the runs - 418-426 episodes/s instead of 429-431; at 1 / 4 episodes per step: 31 -> 42 / 132 -> 159 episodes/s;
# profiles/r04_m_host_enqueue.txt).  Same graph, same kernels, same streams (the engine sets each node's forward stream either way).
# GIM_MT_AUTOGRAD=1 restores torch's default.
_CALLER_THREAD_BACKWARD = os.environ.get("GIM_MT_AUTOGRAD") is None


def caller_thread_backward():
    """Context for .backward() / autograd.grad() calls of the training step: autograd's nodes run on the calling thread."""
    return torch.autograd.set_multithreading_enabled(not _CALLER_THREAD_BACKWARD)


_PENDING_JOIN = []   # streams of lane-1 work the caller's stream has not waited for yet (gim_step(defer_join=True))


def defer_join(stream):
    _PENDING_JOIN.append(stream)


def join_lanes():
    """Make the current stream wait for lane work whose join was deferred.  Called before anything reads what the
    discriminator step wrote: its weights (the next generator step's D forward), its outputs, a checkpoint."""
    if _PENDING_JOIN:
        cur = torch.cuda.current_stream()
        for st in _PENDING_JOIN:
            stream_wait(cur, st)
        del _PENDING_JOIN[:]


class lane:
    """Context manager: work issued inside belongs to lane `idx` (host-side selection, read by the autograd worker)."""

    def __init__(self, idx):
        self.idx = idx

    def __enter__(self):
        self.prev = _LANE[0]
        _LANE[0] = self.idx

    def __exit__(self, *exc):
        _LANE[0] = self.prev


# --------------------------------------------------------------------------------------------
# convolution / linear
# --------------------------------------------------------------------------------------------
class ConvGeom(collections.namedtuple("ConvGeom", "N H W Cin Cout KH ups pre_slope has_bias has_res pool fold res_ups x_act linear key")):
    """One convolution call (a linear: H = W = KH = 1), as every launch of its forward and backward reads it; ConvFn keeps it as
    ctx.cfg.  (H, W): the resolution the unfused conv would run at (after the nearest upsample, before the average pool).
    fold: the launches read the (KH+1)^2-tap folded weights (the pool / sub-pixel forms).  x_act: x is stored ACTIVATED (its
    producer applied this conv's LeakyReLU in its epilogue): forward and wgrad then run without the per-tap activation; dgrad
    keeps the slope - its mask only needs the sign, which is the same.  key = (N, H, W, Cin, Cout, KH, ups, pool, fold): what the
    launch-plan cache, _TUNE_OVERRIDE and count_flops are keyed by."""
    __slots__ = ()

    @classmethod
    def make(cls, N, H, W, Cin, Cout, KH, ups=0, pre_slope=1.0, pool=False, res_ups=False, has_bias=False, has_res=False, x_act=False, linear=False):
        fold = 1 if (pool or (ups and KH > 1)) else 0
        return cls(N, H, W, Cin, Cout, KH, ups, pre_slope, has_bias, has_res, bool(pool), fold, bool(res_ups), bool(x_act), linear,
                   (N, H, W, Cin, Cout, KH, ups, 1 if pool else 0, fold))

    @classmethod
    def of(cls, x, w, ups, pre_slope, pool, res_ups, bias, res, x_act):
        """The call ConvFn.forward(x, w, ...) describes (x NHWC [N, Hs, Ws, Cin], or [N, Cin] with a 2-D weight: a linear)."""
        N, Hs, Ws, Cin = (x.shape[0], 1, 1, x.shape[1]) if x.dim() == 2 else x.shape
        if w.shape[1] != Cin:
            raise RuntimeError("conv: weight expects %d input channels, got %d" % (w.shape[1], Cin))
        return cls.make(N, Hs << ups, Ws << ups, Cin, w.shape[0], w.shape[2] if w.dim() == 4 else 1, ups, pre_slope, pool, res_ups,
                        bias is not None, res is not None, x_act, x.dim() == 2)

    out_pixels = property(lambda s: s.N * (s.H >> s.pool) * (s.W >> s.pool))     # pixels of y / dy
    out_shape = property(lambda s: (s.N, s.Cout) if s.linear else (s.N, s.H >> s.pool, s.W >> s.pool, s.Cout))
    K = property(lambda s: s.KH * s.KH * s.Cin)
    KFF = property(lambda s: (s.KH + 1) * (s.KH + 1) * s.Cin if s.fold else s.K)   # per output channel, in the form the launches read

    def shape(self, kind, pre_slope=None):
        """The caller's own gim_conv_shape for a launch of `kind` ("fwd" / "dgrad" / "wgrad" of _TUNE_OVERRIDE; None: no override)."""
        return _tuned(_shape(self.N, self.H, self.W, self.Cin, self.Cout, self.KH, self.ups, self.pre_slope if pre_slope is None else pre_slope,
                             self.key[7], self.fold, 1 if self.res_ups else 0), kind, self.key)

    def box(self):
        """The forward / wgrad launches of this POOLED 3x3 call on the box-filtered input p [N, H+1, W+1, Cin] (gim_conv_shape.pool = 2:
        the conv's own 9 taps, plain weight layout) - a key of its own for the plan cache, _TUNE_OVERRIDE and count_flops."""
        return self._replace(fold=0, pre_slope=1.0, key=self.key[:7] + (2, 0))

    def linear_map(self):
        """The conv as a linear map of its input: no prologue, bias or residual (ConvDgradFn's adjoints)."""
        return ConvGeom.make(self.N, self.H, self.W, self.Cin, self.Cout, self.KH, 0, 1.0, self.pool, linear=self.linear)


# The _*_route functions decide which kernel a launch takes, for the product and the tools; only they read the switches
_ACT_STORAGE = os.environ.get("GIM_NO_ACT_STORAGE") is None   # A/B switch (host side)
_ROWS_FORM = os.environ.get("GIM_NO_ROWS_FORM") is None   # row-contiguous K for the image layers
_MERGED_SUBPIXEL = os.environ.get("GIM_NO_MERGED_SUBPIXEL") is None   # stacked parity classes for the 9x9 64->3 layer
_NARROW_DGRAD_T = os.environ.get("GIM_NO_NARROW_DGRAD_T") is None
_NARROW_XFOLD = os.environ.get("GIM_NO_NARROW_XFOLD") is None
_BOX_POOL = os.environ.get("GIM_NO_BOX_POOL") is None   # pooled 3x3 convs: forward / wgrad on the box-filtered input (9 taps, not the fold's 16)


def _fwd_route(g, tune_tile):
    """"rows" (image layers: row-contiguous K on a zero-padded, activated copy of the image, gim_conv2d_fwd_rows), "subpixel" (the
    generator's 9x9 64->3 layer behind the upsample: the four output-parity classes as ONE plain 5-tap convolution to 4 * Cout channels
    + a depth-to-space copy) or "plain" (gim_conv2d_fwd).  tune_tile: of the launch's gim_conv_shape - an override keeps "plain"."""
    if g.linear or tune_tile != 0:
        return "plain"
    if _ROWS_FORM and g.KH >= 3 and g.Cin <= 8 and g.KH * g.Cin <= 64 and g.Cout >= 16 and g.Cout % 4 == 0 and not (g.ups or g.pool or g.res_ups):
        return "rows"
    if _MERGED_SUBPIXEL and g.ups and g.KH >= 5 and (g.KH & 3) == 1 and g.Cout <= 4 and not g.has_res:
        return "subpixel"
    return "plain"


def _pool_route(g, prec, tune_tile=0):
    """Forward and weight gradient of a pooled convolution: "fold" (ONE stride-2 conv over the (K+1)^2 folded taps of x) or "box" (a
    streaming 2x2 box filter of the zero-padded activated x - gim_box2_fwd - then ONE stride-2 conv with the conv's own 9 taps:
    9/36 instead of 16/36 of the unfused FLOPs; the weight gradient reads the saved box map).  Eligible: 3x3, gathered channels % 16
    == 0 (16-byte loads), fp32 matrix path (`prec` 0), no launch override on the folded key (`tune_tile`).  The input gradient keeps
    the fold on either route (its box form would need an odd-sized (H+1) x (W+1) output grid)."""
    if not (_BOX_POOL and g.pool) or g.linear or g.ups or g.KH != 3 or g.Cin % 16 != 0 or prec != 0 or tune_tile != 0:
        return "fold"
    return "box"


def _fwd_launch(g, tap_slope=None):
    """-> (geometry, gim_conv_shape) of the forward launch of g: g.box() where _pool_route says "box", else g itself."""
    sh = g.shape("fwd", tap_slope)
    # (a launch override on the folded key, forward or weight gradient, asks for the folded launches)
    if g.pool and _pool_route(g, sh.prec, sh.tune_tile or (1 if ("wgrad", g.key) in _TUNE_OVERRIDE else 0)) == "box":
        g = g.box()
        sh = g.shape("fwd")
    return g, sh


def _xfold_factor(Cin, W):
    """J of the x-folded dgrad, dividing W.  Cin <= 4: J = 4 -> up to 16 output columns, the 16-column MFMA tile (12 of 16 carry data
    for RGB).  Cin = 5, 6 (the generator's 6-channel image pair): J = 4 -> 24 columns on the 32-column tile of
    v_mfma_f32_32x32x2_f32 instead of 12 on the 16-column tile of the 16 x 16 x 4 form (the same peak rate, but twice the LDS operand
    reads per FLOP and a quarter of the work per instruction): 20 % more taps (K + 3 instead of K + 1 columns) and still
    0.51 -> 0.32 ms on the 9x9 64->6 gradient (round 4).  Cin = 7, 8: J = 2."""
    J = 4 if Cin <= 6 else 2
    return J if (Cin <= 8 and W % J == 0 and W // J >= 1) else 0


def _dgrad_route(g, prec, has_w, has_res_half=False):
    """-> (route, J, add_res) on matrix path `prec` (gim_conv_shape.prec); has_w: the caller has the weight PARAMETER, whose cached
    re-laid-out copies the first two routes read.  "t": gim_conv2d_dgrad_t on transposed weights (rows k-contiguous: vector weight loads)
    for the gradient w.r.t. IMAGES (<= 8 input channels), where the k-major kernel loads weights as scalars - and EVERY eligible dgrad
    of the fp16 path, whose kernel exists in this form only; "xfold": those image layers when plain, J adjacent dx pixels as the output
    columns of one stride-(1, J) convolution; "ups": 1x1 behind up2; "plain".  has_res_half (0.25 * up2(res_half) is to be added):
    "res", the plain form with the addition in its epilogue - or the launch's own route and add_res (gim_add_avgpool2_bwd follows)."""
    f16_t = prec >= 1 and g.Cout % 32 == 0 and g.Cin >= 32
    J = 0
    if has_w and g.Cout % 16 == 0 and not (g.ups and not g.fold) and ((g.Cin <= 8 and _NARROW_DGRAD_T) or f16_t):
        if g.KH >= 3 and not (g.ups or g.pool or g.fold) and _NARROW_XFOLD and not f16_t:
            J = _xfold_factor(g.Cin, g.W)
        route = "xfold" if J else "t"
    else:
        route = "ups" if (g.ups and not g.fold) else "plain"
    if not has_res_half:
        return route, J, False
    if route == "plain" and not (g.pool or g.fold) and g.pre_slope != 1.0 and not f16_t:
        return "res", 0, False
    return route, J, True


def _wgrad_route(g, sh, has_target, has_sigma, bias_untargeted=False, rows_copy=False):
    """-> (route, slabs).  has_target: the parameter's .grad can be added into (_grad_target); bias_untargeted: a bias gradient is
    wanted from the same launch but has no such buffer; rows_copy: the "rows" forward left its padded copy and dy is contiguous.
    "queued" / "queued_rows": raw gradient into an arena slot now, all convs finished by two launches when backward ends (WgradQueue);
    "direct": one gim_conv2d_wgrad writes the gradient; "slabs": `slabs` slabs (GIM_WGRAD_SLABS / deterministic mode: as many as the
    library says, added in a fixed order) + gim_wgrad_finish."""
    if has_target and wgrad_queue.enabled and not _DETERMINISTIC[0] and not bias_untargeted:
        return ("queued_rows" if rows_copy else "queued"), 1
    ns = 1
    if _WGRAD_SLABS or _DETERMINISTIC[0]:
        ns = _lib.load().gim_conv2d_wgrad_slabs(sh)
        if ns <= 0:
            check(ns, "conv2d_wgrad_slabs")
    return ("direct" if (ns == 1 and not has_sigma and not g.fold and not has_target) else "slabs"), ns


def _stores_activated(g, post_slope):
    """Does the forward of g write lrelu(y, post_slope)?  (Not a split-K launch; "subpixel" activates in its depth-to-space copy.)"""
    if not (_ACT_STORAGE and post_slope != 1.0) or g.linear:
        return False
    gl, sh = _fwd_launch(g)
    return _fwd_route(g, sh.tune_tile) == "subpixel" or _launch_plan(sh, 0, gl.key).ksplit == 1


def _merged_subpixel(x, w, ups, res, sh):
    """Does this forward run as the stacked-parity-class convolution ("subpixel" of _fwd_route)?"""
    return _fwd_route(ConvGeom.of(x, w, ups, 1.0, False, False, None, res, False), sh.tune_tile) == "subpixel"


class ConvFn(Function):
    """y = [avgpool2]( conv(up2^ups(lrelu(x, pre_slope)), w) ) / sigma + bias + res   (NHWC; linear when x is 2-D).
    pool: the 2x2 average pool behind the conv is folded into ONE stride-2 convolution (over the folded taps of x, or - _pool_route
    "box": forward and wgrad of 3x3 layers - over the conv's own taps of the box-filtered x); ups with a KxK kernel
    (K > 1) runs in its sub-pixel form on the low-resolution input: neither pooling nor upsampling costs conv FLOPs.
    res_ups: the residual is stored at half the output resolution."""
    N_EXTRA = 11    # forward's inputs behind (x, w, bias, res): backward hands None back for each

    @staticmethod
    def forward(ctx, x, w, bias, res, sigma, u_s, v_s, ups, pre_slope, pool, res_ups, wf=None, guard=None, post_slope=1.0, x_act=False):
        lib = _lib.load()
        x = _req(x, "x")
        wp = weight_phys(_req_w(w))
        g = ConvGeom.of(x, w, ups, pre_slope, pool, res_ups, bias, res, x_act)
        N, H, W, Cin, Cout, KH = g.N, g.H, g.W, g.Cin, g.Cout, g.KH
        tap_slope = 1.0 if x_act else pre_slope
        gl, sh = _fwd_launch(g, tap_slope)    # gl is not g: the pooled conv runs on the box-filtered input (_pool_route)
        route = _fwd_route(g, sh.tune_tile)
        # post_slope != 1: store lrelu(y) for the ONLY reader of y, which runs with x_act (callers ask _stores_activated; refused here otherwise)
        if post_slope != 1.0 and route != "subpixel":
            if g.linear or _launch_plan(sh, 0, gl.key).ksplit > 1:
                raise RuntimeError("conv: an activated output (post_slope) cannot be combined with a split-K launch or a linear layer")
            sh.post_slope = post_slope
        if res is not None:
            res = _req(res, "res")
        xp = None
        if route == "rows":
            pad = (KH - 1) // 2
            xp = torch.empty((N, H + 2 * pad, W + 2 * pad, Cin), device=x.device, dtype=torch.float32)
            check(lib.gim_pad_image(_p(x), _p(xp), N, H, W, Cin, pad, tap_slope, _stream()), "pad_image")
            wrows = _transposed(lib, w, wp, Cout, Cin, KH, rows=True)
            sh.tune_ksplit = 1      # one K slice: these layers have >= 10^5 output pixels; keeps an activated output (post_slope) legal
            y = torch.empty(g.out_shape, device=x.device, dtype=torch.float32)
            check(lib.gim_conv2d_fwd_rows(_p(xp), _p(wrows), _p(bias), _p(sigma), _p(res), _p(y), sh, _stream()), "conv2d_fwd_rows")
        elif route == "subpixel":    # (gradients: the sub-pixel forms on the folded weights)
            if wf is None:
                wf = _folded(wp, Cout, Cin, KH)
            wm = _transposed(lib, w, wf, Cout, Cin, KH, subpix=True)
            gm = ConvGeom.make(N, H >> 1, W >> 1, Cin, 4 * Cout, (KH + 1) // 2)
            shm = gm.shape("fwd", tap_slope)
            y4 = _conv_out(shm, 0, gm.key, gm.out_shape, x.device)
            check(lib.gim_conv2d_fwd(_p(x), _p(wm), None, _p(sigma), None, _p(y4), shm, _stream()), "conv2d_fwd")
            y = torch.empty(g.out_shape, device=x.device, dtype=torch.float32)
            check(lib.gim_depth_to_space2(_p(y4), _p(bias), _p(y), N, H >> 1, W >> 1, Cout, post_slope, _stream()), "depth_to_space2")
        elif gl is not g:    # box filter (applies the LeakyReLU unless x is stored activated), then the conv's own 9 taps at stride 2
            xp = torch.empty((N, H + 1, W + 1, Cin), device=x.device, dtype=torch.float32)
            check(lib.gim_box2_fwd(_p(x), _p(xp), N, H, W, Cin, tap_slope, _stream()), "box2_fwd")
            y = _conv_out(sh, 0, gl.key, g.out_shape, x.device)
            check(lib.gim_conv2d_fwd(_p(xp), _p(wp), _p(bias), _p(sigma), _p(res), _p(y), sh, _stream()), "conv2d_fwd")
        else:
            y = _conv_out(sh, 0, g.key, g.out_shape, x.device)
            if g.fold and wf is None:
                wf = _folded(wp, Cout, Cin, KH)
            check(lib.gim_conv2d_fwd(_p(x), _p(wf if g.fold else wp), _p(bias), _p(sigma), _p(res), _p(y), sh, _stream()), "conv2d_fwd")
        ctx.save_for_backward(x, w, sigma, u_s, v_s, wf if g.fold else None, bias, xp)
        ctx.cfg = g
        ctx.guard = guard
        if _FLOPS is not None:
            _note_conv("fwd", gl, sh, 0)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, w, sigma, u_s, v_s, wf, bias, xp = ctx.saved_tensors
        g = ctx.cfg
        dy = _req(dy, "dy")
        if ctx.guard is not None and ctx.guard[0].stale(ctx.guard[1]):
            raise RuntimeError("the spectral-norm state (sigma, u, v) of this forward pass was overwritten by later forward "
                               "passes of the same model: run backward before the third forward")
        need = ctx.needs_input_grad
        box = g.pool and xp is not None     # forward on the box-filtered input xp: the weight gradient reads it, the input gradient keeps the fold
        if g.fold and wf is None and need[0]:
            with torch.no_grad():
                wf = _folded(weight_phys(w), g.Cout, g.Cin, g.KH)
        if _second_order():
            if g.ups or g.res_ups:
                raise NotImplementedError("second-order backward of an upsampling convolution is not on the R1 path")
            dx = ConvDgradFn.apply(dy, w, x, sigma, u_s, v_s, wf, g) if need[0] else None
            return (dx, None, None, dy if g.has_res and need[3] else None) + (None,) * ConvFn.N_EXTRA
        wp = weight_phys(w)
        st = _stream()
        dev = dy.device
        dx = dw = db = dres = None
        if need[0]:
            dx = _conv_dgrad(lib, dy, x, wp, wf, sigma, g.shape("dgrad"), g, st, w, getattr(ctx, "dgrad_res", None))
        want_b = g.has_bias and need[2]
        if need[1] and box:
            gb = g.box()
            dw, db = _conv_wgrad(lib, dy, xp, w, wp, bias, sigma, u_s, v_s, gb.shape("wgrad"), gb, want_b, st)
        elif need[1]:     # (x_act: the stored x is already lrelu(x): no activation on the wgrad operand)
            dw, db = _conv_wgrad(lib, dy, x, w, wp, bias, sigma, u_s, v_s, g.shape("wgrad", 1.0 if g.x_act else None), g, want_b, st, xp)
        elif want_b:
            db = torch.empty(g.Cout, device=dev, dtype=torch.float32)
            scratch = torch.empty(256 * g.Cout, device=dev, dtype=torch.float32)
            check(lib.gim_colsum(_p(dy), _p(db), _p(scratch), g.out_pixels, g.Cout, st), "colsum")
        if g.has_res and need[3]:
            if g.res_ups:
                dres = torch.empty((g.N, g.H >> 1, g.W >> 1, g.Cout), device=dev, dtype=torch.float32)
                check(lib.gim_upsample2x_bwd(_p(dy), None, 1.0, _p(dres), g.N, g.H >> 1, g.W >> 1, g.Cout, st), "upsample2x_bwd")
            else:
                dres = dy
        return (dx, dw, db, dres) + (None,) * ConvFn.N_EXTRA


class _DerivedWeights(_StreamReady):
    """One entry of _WT_CACHE; version: of the weights it was made from, param: weak reference to the parameter."""
    __slots__ = ("version", "param")


class _DerivedWeightCache(dict):
    """Copies of a parameter's weights in another layout (_transposed's four, SNConv2d's "fold"), one per (parameter storage,
    slot = (taps per dim, layout)), each valid while the weights are what it was made from: the same parameter object, autograd
    version counter (torch-side writes) and optim.weights_epoch (the fused Adam kernel).  Entries leave with their parameter."""

    def _fresh(self, w, slot):
        ent = dict.get(self, (w.data_ptr(),) + slot)
        return ent if ent is not None and ent.version == (w._version, optim.weights_epoch(w)) and ent.param() is w else None

    def is_stale(self, w, slot):
        return self._fresh(w, slot) is None

    def install(self, w, slot, tensor):
        """`tensor` was just written on the current stream from w's weights as they are now (by `make` of get, or elsewhere)."""
        key = (w.data_ptr(),) + slot
        ent = self[key] = _DerivedWeights(tensor)
        ent.version, ent.param = (w._version, optim.weights_epoch(w)), weakref.ref(w, lambda _r: self.pop(key, None))
        return ent

    def get(self, w, slot, make, raw=None):
        """The copy in `slot`, made by make() if there is none of the current weights, ready for use on the current stream (raw)."""
        ent = self._fresh(w, slot)
        if ent is None:
            with torch.no_grad():
                ent = self.install(w, slot, make())
        return ent.use_on_current_stream(raw)


_WT_CACHE = _DerivedWeightCache()


def _transposed(lib, w, wk, Cout, Cin, KF, xfold=0, rows=False, subpix=False):
    """WT[Cin][KF][KF][Cout] of the (plain or folded) weights `wk` of parameter `w` - or, xfold = J, the x-folded
    WX[J * Cin][KF][KF + J - 1][Cout] of gim_conv2d_xfold_weights; or, rows, the row-padded WP[Cout][KF][KF * Cin -> 16] of
    gim_conv2d_pack_rows_weights; or, subpix (wk = the folded taps, KF = the conv's K), the stacked parity classes
    WM[4 Cout][(KF+1)/2][(KF+1)/2][Cin] of gim_conv2d_pack_subpixel_weights - from _WT_CACHE: made again only when the weights changed."""
    raw = _stream()

    def run(fn, n, what, *tail):
        wt = torch.empty(n, device=wk.device, dtype=torch.float32)
        check(fn(_p(wk), _p(wt), Cout, Cin, KF, *tail, raw), what)
        return wt
    if rows:
        layout, make = "rows", lambda: run(lib.gim_conv2d_pack_rows_weights, Cout * KF * ((KF * Cin + 15) & ~15), "pack_rows_weights")
    elif subpix:
        layout, make = "subpix", lambda: run(lib.gim_conv2d_pack_subpixel_weights, 4 * Cout * ((KF + 1) // 2) ** 2 * Cin, "pack_subpixel_weights")
    elif xfold:
        layout, make = xfold, lambda: run(lib.gim_conv2d_xfold_weights, xfold * Cin * KF * (KF + xfold - 1) * Cout, "xfold_weights", xfold)
    else:
        layout, make = 0, lambda: run(lib.gim_conv2d_transpose_weights, Cin * KF * KF * Cout, "transpose_weights")
    return _WT_CACHE.get(w, (KF, layout), make, raw)


def _conv_dgrad(lib, dy, x, wp, wf, sigma, sh, g, st, w=None, res_half=None):
    """dx = lrelu'(x) * dgrad(dy, w) / sigma  (through the pool / sub-pixel folds when the forward used them), by the route
    _dgrad_route names.  w: the weight parameter, where the caller has it.
    res_half [N, H/2, W/2, Cin]: the gradient w.r.t. avgpool2(x) of a second reader of x (ConvForkPoolFn): 0.25 * up2(res_half) is added."""
    route, J, add_res = _dgrad_route(g, sh.prec, w is not None, res_half is not None)
    if _FLOPS is not None:
        _note_conv("dgrad", g, sh, 1)
    N, H, W, Cin, Cout, KH = g.N, g.H, g.W, g.Cin, g.Cout, g.KH
    mask = x if g.pre_slope != 1.0 else None
    wk = wf if g.fold else wp
    if route == "xfold":
        wx = _transposed(lib, w, wk, Cout, Cin, KH, xfold=J)
        dx = torch.empty(tuple(x.shape), device=x.device, dtype=torch.float32)
        check(lib.gim_conv2d_dgrad_xfold(_p(dy), _p(wx), _p(sigma), _p(mask), _p(dx), sh, J, st), "conv2d_dgrad_xfold")
    elif route == "t":
        wt = _transposed(lib, w, wk, Cout, Cin, KH + 1 if g.fold else KH)
        dx = _conv_out(sh, 2, g.key, tuple(x.shape), x.device)
        check(lib.gim_conv2d_dgrad_t(_p(dy), _p(wt), _p(sigma), _p(mask), _p(dx), sh, st), "conv2d_dgrad_t")
    elif route == "ups":
        dxu = _conv_out(sh, 1, g.key, (N, H, W, Cin), dy.device)
        dx = torch.empty_like(x)
        check(lib.gim_conv2d_dgrad(_p(dy), _p(wk), _p(sigma), None, _p(dxu), sh, st), "conv2d_dgrad")
        check(lib.gim_upsample2x_bwd(_p(dxu), _p(mask), g.pre_slope, _p(dx), N, H >> 1, W >> 1, Cin, st), "upsample2x_bwd")
    else:
        dx = _conv_out(sh, 1, g.key, tuple(x.shape), x.device)
        if route == "res":
            check(lib.gim_conv2d_dgrad_res(_p(dy), _p(wk), _p(sigma), _p(mask), _p(_req(res_half, "res_half")), 0.25, _p(dx), sh, st), "conv2d_dgrad_res")
        else:
            check(lib.gim_conv2d_dgrad(_p(dy), _p(wk), _p(sigma), _p(mask), _p(dx), sh, st), "conv2d_dgrad")
    if add_res:
        out = torch.empty_like(dx)
        check(lib.gim_add_avgpool2_bwd(_p(dx), _p(_req(res_half, "res_half")), _p(out), N, H, W, Cin, st), "add_avgpool2_bwd")
        return out
    return dx


def _conv_wgrad(lib, dy, x, w, wp, bias, sigma, u_s, v_s, sh, g, want_b, st, xp=None):
    """(dw, db) of one convolution, by the route _wgrad_route names; either may come back None because it was ADDED into the
    parameter's .grad.  xp: the padded, activated copy of x that a forward in the row-contiguous form made (image layers)."""
    if _FLOPS is not None:
        _note_conv("wgrad", g)
    Cin, Cout, KH, ups, fold = g.Cin, g.Cout, g.KH, g.ups, g.fold
    dev = dy.device
    dw = db = None
    Mo, K, KFF = g.out_pixels, g.K, g.KFF
    slab_bias = want_b and not (fold and ups)  # the role-swapped sub-pixel wgrad does not stream dy as its A operand
    # Megatron-style direct accumulation: when the parameter's .grad already exists as a dense buffer in the
    # weight's own memory order (FusedAdam's flat gradient bucket) and no higher-order graph is being built,
    # the finish kernels ADD into it and autograd gets None (no AccumulateGrad add kernel per parameter).
    acc_w = _grad_target(w) if (sigma is not None or not fold) and not torch.is_grad_enabled() else None
    acc_b = _grad_target(bias) if (slab_bias and acc_w is not None) else None
    route, ns = _wgrad_route(g, sh, acc_w is not None, sigma is not None, want_b and slab_bias and acc_b is None,
                             xp is not None and dy.is_contiguous())
    fold_code = (2 if ups else 1) if fold else 0    # gim_wgrad_finish*: how the finish un-folds the raw gradient
    queued = route in ("queued", "queued_rows")
    if queued:
        q = _queue()
        n = Cout * K
        if Cout * KFF >= 1 << 31:
            raise RuntimeError("weight gradient of more than 2^31 elements (gim_wgrad_finish_batched indexes with 32 bits)")
        n_chunks = (n + q.CHUNK - 1) // q.CHUNK
        rows = route == "queued_rows"
        src = q.take(Cout * KH * ((KH * Cin + 15) & ~15) if rows else Cout * KFF, dev)
        bsrc = q.take(Cout, dev) if slab_bias else None
        sn = sigma is not None
        tmp = q.take(n, dev) if ((fold or rows) and sn) else None
        part = q.take(n_chunks, dev) if sn else None
        if rows:   # slot [Cout][KH][KH * Cin -> 16]; the batched finish un-pads it (fold code 3)
            check(lib.gim_conv2d_wgrad_rows_acc(_p(dy), _p(xp), src, bsrc, sh, st), "conv2d_wgrad_rows_acc")
        else:
            check(lib.gim_conv2d_wgrad_acc(_p(dy), _p(x), src, bsrc, sh, st), "conv2d_wgrad_acc")
        q.add((src, bsrc or 0, _p(wp) if sn else 0, _p(sigma) or 0, _p(u_s) or 0, _p(v_s) or 0, tmp or 0, part or 0,
               _p(acc_w), _p(acc_b) or 0, Cout, Cin, KH, 3 if rows else fold_code, n_chunks), (sigma, u_s, v_s))
    else:
        dwp = torch.empty(Cout * K, device=dev, dtype=torch.float32)
        if want_b and acc_b is None:
            db = torch.empty(Cout, device=dev, dtype=torch.float32)
        if route == "direct":
            check(lib.gim_conv2d_wgrad(_p(dy), _p(x), _p(dwp), _p(db) if slab_bias else None, 1, sh, st), "conv2d_wgrad")
        else:
            slabs = torch.empty(ns * Cout * KFF, device=dev, dtype=torch.float32)
            bslabs = torch.empty(ns * Cout, device=dev, dtype=torch.float32) if slab_bias else None
            scratch = torch.empty(512 + (Cout * KFF if fold else 0), device=dev, dtype=torch.float32)
            check(lib.gim_conv2d_wgrad(_p(dy), _p(x), _p(slabs), _p(bslabs), ns, sh, st), "conv2d_wgrad")
            check(lib.gim_wgrad_finish(_p(slabs), _p(bslabs), ns, _p(wp), _p(sigma), _p(u_s), _p(v_s), _p(dwp),
                                       _p(db) if (slab_bias and acc_b is None) else None, _p(scratch), Cout, Cin, KH,
                                       fold_code, _p(acc_w), _p(acc_b), st), "wgrad_finish")
        if acc_w is None:
            dw = dwp.view(Cout, KH, KH, Cin).permute(0, 3, 1, 2) if w.dim() == 4 else dwp.view(Cout, Cin)
    if want_b and not slab_bias:    # the bias gradient as a column sum of dy of its own (queued: into .grad where that exists)
        scr = torch.empty(256 * Cout, device=dev, dtype=torch.float32)
        tgt_b = _grad_target(bias) if queued else None
        if tgt_b is not None:
            check(lib.gim_colsum_acc(_p(dy), _p(tgt_b), _p(scr), Mo, Cout, st), "colsum_acc")
        else:
            if db is None:
                db = torch.empty(Cout, device=dev, dtype=torch.float32)
            check(lib.gim_colsum(_p(dy), _p(db), _p(scr), Mo, Cout, st), "colsum")
    return dw, db


class ConvDgradFn(Function):
    """The first-order input gradient of ConvFn as an operator of (dy, w):  dx = lrelu'(x) * conv^T(dy, w / sigma(w)).
    It is bilinear in (dy, w/sigma), so its own adjoints are the other two kernels of the same convolution:
    d/d(dy) is the FORWARD conv of the masked cotangent and d/dw is the WGRAD with that cotangent in the role of
    the layer input (followed by the same spectral-norm chain rule).  The mask is piecewise constant in x.  (geom: ConvFn's, never upsampling.)"""
    N_EXTRA = 6    # forward's inputs behind (dy, w)

    @staticmethod
    def forward(ctx, dy, w, x, sigma, u_s, v_s, wf, geom):
        dx = _conv_dgrad(_lib.load(), dy, x, weight_phys(w), wf, sigma, geom.shape(None), geom, _stream(), w)
        ctx.save_for_backward(dy, w, x, sigma, u_s, v_s, wf)
        ctx.cfg = geom
        return dx

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        dy, w, x, sigma, u_s, v_s, wf = ctx.saved_tensors
        geom = ctx.cfg
        if torch.is_grad_enabled():
            raise NotImplementedError("third-order gradients are not supported")
        g = _req(g, "g")
        st = _stream()
        wp = weight_phys(w)
        if geom.pre_slope != 1.0:
            gm = torch.empty_like(g)
            check(lib.gim_lrelu_mask_mul(_p(g), _p(x), geom.pre_slope, _p(gm), g.numel(), st), "lrelu_mask_mul")
        else:
            gm = g
        lin = geom.linear_map()
        sh = lin.shape(None)
        g_dy = g_w = None
        if ctx.needs_input_grad[0]:
            g_dy = torch.empty_like(dy)
            check(lib.gim_conv2d_fwd(_p(gm), _p(wf if lin.fold else wp), None, _p(sigma), None, _p(g_dy), sh, st), "conv2d_fwd")
            if _FLOPS is not None:
                _note_conv("fwd", lin, sh, 0)
        if ctx.needs_input_grad[1]:
            g_w, _ = _conv_wgrad(lib, dy, gm, w, wp, None, sigma, u_s, v_s, sh, lin, False, st)
        return (g_dy, g_w) + (None,) * ConvDgradFn.N_EXTRA


def _grad_target(p):
    """The parameter's existing .grad as a flat buffer in the parameter's own memory order, or None.  (The checked view is kept
    on the gradient tensor, keyed by its data pointer - FusedAdam's gradients are fixed views of its flat bucket.)"""
    if p is None:
        return None
    g = p.grad
    if g is None:
        return None
    try:
        c = g._gim_tgt
        if c[0] == g.data_ptr():
            return c[1]
    except AttributeError:
        pass
    if not g.is_cuda or g.dtype != torch.float32 or g.shape != p.shape:
        return None
    gp = g.permute(0, 2, 3, 1) if g.dim() == 4 else g
    if not gp.is_contiguous():
        return None
    g._gim_tgt = (g.data_ptr(), gp)
    return gp


def _req_w(w):
    if not (w.is_cuda and w.dtype == torch.float32):
        raise RuntimeError("weights must be CUDA float32 (got %s on %s): the GIM engine has no CPU path" % (w.dtype, w.device))
    return w


def conv2d(x, w, bias=None, res=None, sigma=None, u_s=None, v_s=None, ups=0, pre_slope=1.0, pool=False, res_ups=False, wf=None,
           guard=None, x_act=False):
    return ConvFn.apply(x, w, bias, res, sigma, u_s, v_s, ups, pre_slope, pool, res_ups, wf, guard, 1.0, x_act)


def conv2d_post_act(x, w, bias=None, res=None, sigma=None, u_s=None, v_s=None, ups=0, pre_slope=1.0, pool=False, res_ups=False, wf=None,
                    guard=None, post_slope=1.0, x_act=False):
    """conv2d whose output may be stored ACTIVATED, y_stored = lrelu(y, post_slope), for a consumer conv that is the only reader
    of y and is then called with x_act=True (it skips its per-tap LeakyReLU in forward and wgrad; its dgrad masks by the sign,
    which activation does not change, and hands back the gradient w.r.t. the RAW y - so this conv's backward is unchanged).
    Returns (y_stored, activated): launches that split K cannot activate (their slices combine by addition) and return raw y.
    Decided HERE, for this call's own shape, and handed to ConvFn as the resolved slope: nothing about the stored form of y
    travels through module state (another conv running in between could not change what this call reports)."""
    act = post_slope != 1.0 and _stores_activated(ConvGeom.of(x, w, ups, pre_slope, pool, res_ups, bias, res, x_act), post_slope)
    y = ConvFn.apply(x, w, bias, res, sigma, u_s, v_s, ups, pre_slope, pool, res_ups, wf, guard, post_slope if act else 1.0, x_act)
    return y, act


class ConvForkPoolFn(Function):
    """(y, pooled) = (ConvFn(x, w, ...), avgpool2(raw x)) for the TWO readers of a ResBlockDown's input (models/model_blocks.py:497-514:
    conv_r1 behind a LeakyReLU, the 1x1 skip conv on the pooled input).  Forward = the two launches they always were; backward = ONE
    dgrad launch whose epilogue adds 0.25 * up2(d pooled) to the masked conv gradient (gim_conv2d_dgrad_res) - round 3 summed the two
    branches in a kernel of its own (gim_add_avgpool2_bwd: a read-modify-write of the block's whole input gradient, 36 launches and
    0.58 ms per training step).  Inputs = ConvFn's, in ConvFn's order (so that ConvFn.backward's bookkeeping applies as it is), plus
    in_slope (x stored activated: the pool inverts the LeakyReLU on the fly, see AvgPool2Fn)."""

    @staticmethod
    def forward(ctx, x, w, bias, res, sigma, u_s, v_s, ups, pre_slope, pool, res_ups, wf, guard, post_slope, x_act, in_slope):
        x, pooled = _avgpool2(x, in_slope)
        y = ConvFn.forward(ctx, x, w, bias, None, sigma, u_s, v_s, 0, pre_slope, False, False, None, guard, post_slope, x_act)
        return y, pooled

    @staticmethod
    def backward(ctx, dy, dpooled):
        x_shape = (ctx.cfg.N, ctx.cfg.H, ctx.cfg.W, ctx.cfg.Cin)
        if dy is None:      # the conv branch is unused: only the pool's backward
            return (AvgPool2BwdFn.apply(dpooled, x_shape) if dpooled is not None else None,) + (None,) * (3 + ConvFn.N_EXTRA + 1)
        if dpooled is not None and (torch.is_grad_enabled() or not ctx.needs_input_grad[0]):
            # second-order pass (R1) - or no input gradient wanted at all: the unfused sum of differentiable pieces
            grads = ConvFn.backward(ctx, dy)
            gp = AvgPool2BwdFn.apply(dpooled, x_shape) if ctx.needs_input_grad[0] else None
            dx = gp if grads[0] is None else (grads[0] if gp is None else grads[0] + gp)
            return (dx,) + grads[1:] + (None,)
        ctx.dgrad_res = dpooled
        try:
            grads = ConvFn.backward(ctx, dy)
        finally:
            ctx.dgrad_res = None
        return grads + (None,)


_FUSED_FORKPOOL = os.environ.get("GIM_NO_FUSED_FORKPOOL") is None   # A/B switch (host side)


def conv2d_forkpool(x, w, bias, sigma, u_s, v_s, pre_slope, guard, post_slope, x_act, in_slope):
    """-> (y_stored, activated, pooled): conv2d_post_act of a plain convolution plus avgpool2 of its (raw) input, as ONE autograd node
    whose backward folds the pooled branch's gradient into the dgrad epilogue (ConvForkPoolFn)."""
    act = post_slope != 1.0 and _stores_activated(ConvGeom.of(x, w, 0, pre_slope, False, False, bias, None, x_act), post_slope)
    ps = post_slope if act else 1.0
    if _FUSED_FORKPOOL and x.requires_grad and torch.is_grad_enabled():
        y, pooled = ConvForkPoolFn.apply(x, w, bias, None, sigma, u_s, v_s, 0, pre_slope, False, False, None, guard, ps, x_act, in_slope)
    else:
        xa, pooled = fork_pool(x, in_slope)
        y = ConvFn.apply(xa, w, bias, None, sigma, u_s, v_s, 0, pre_slope, False, False, None, guard, ps, x_act)
    return y, act, pooled


def linear(x, w, bias=None, pre_slope=1.0):
    """nn.Linear on the last dim (optionally with a fused LeakyReLU on the input)."""
    shp = x.shape
    y = ConvFn.apply(x.reshape(-1, shp[-1]), w, bias, None, None, None, None, 0, pre_slope, False, False, None, None)
    return y.view(*shp[:-1], w.shape[0])


# --------------------------------------------------------------------------------------------
# grouped linears (many nn.Linear on one shared input: the style projections of the AdaIN blocks)
# --------------------------------------------------------------------------------------------
_GEMM_TABLES = _TableCache("grouped linears", 64)


def _gemm_tables(jobs, col_tiles_only=False, raw=None):
    """(device job table, device tile table, tiles) of a grouped launch on stream `raw` (include/gim_hip.h gim_gemm_job)."""
    def build():
        arr = (GimGemmJob * len(jobs))(*jobs)
        tiles = [(j, it, jt) for j, jb in enumerate(jobs) for it in range(1 if col_tiles_only else (jb[4] + 63) // 64)
                 for jt in range((jb[5] + 63) // 64)]
        return _DeviceTable(arr, tiles, extra=len(tiles))
    ent = _GEMM_TABLES.get((tuple(jobs), col_tiles_only), build)
    ent.use_on_current_stream(raw)
    return ent.ptrs[0], ent.ptrs[1], ent.extra


class GroupedLinearFn(Function):
    """(y_0, ..., y_{n-1}) with y_g = x @ w_g^T + b_g for n nn.Linear layers on ONE input x [M, K]: one launch forward, and one
    grouped product + one grouped column sum backward (dx = sum_g dy_g @ w_g with float atomics into a zeroed buffer, dw_g =
    dy_g^T @ x and db_g added straight into the optimizer's gradient bucket where it exists).  Replaces 3 x n launches of 5-7 us
    (the 36 style projections of the generator: models/model_blocks.py:786-789,829-832) and the n - 1 autograd additions of dx."""

    @staticmethod
    def forward(ctx, x, *wb):
        lib = _lib.load()
        x = _req(x, "x")
        M, K = x.shape
        ws, bs = wb[0::2], wb[1::2]
        for w in ws:
            if not (w.is_cuda and w.dtype == torch.float32 and w.dim() == 2 and w.shape[1] == K and w.is_contiguous()):
                raise RuntimeError("grouped linear: weights must be contiguous CUDA float32 [out, %d]" % K)
        sizes = [w.shape[0] for w in ws]
        buf = torch.empty(M * sum(sizes), device=x.device, dtype=torch.float32)
        ys, off = [], 0
        for n_ in sizes:
            ys.append(buf[off:off + M * n_].view(M, n_))
            off += M * n_
        jobs = [(_p(x), _p(w), _p(y), _p(b) or 0, M, n_, K, n_, K, 1, 1, K, 0) for w, b, y, n_ in zip(ws, bs, ys, sizes)]
        st = _stream()
        check(lib.gim_bgemm_grouped(*_gemm_tables(jobs, raw=st), st), "bgemm_grouped")
        for n_ in sizes:
            _note_bgemm(1, M, n_, K)
        ctx.save_for_backward(x, *wb)
        return tuple(ys)

    @staticmethod
    @once_differentiable
    def backward(ctx, *dys):
        lib = _lib.load()
        x, *wb = ctx.saved_tensors
        ws, bs = wb[0::2], wb[1::2]
        M, K = x.shape
        st = _stream()
        need_x = ctx.needs_input_grad[0]
        dx = torch.zeros((M, K), device=x.device, dtype=torch.float32) if need_x else None
        jobs, cjobs, grads = [], [], []
        for g, (w, b, dy) in enumerate(zip(ws, bs, dys)):
            gw = gb = None
            if dy is not None:
                dy = _req(dy, "dy")
                n_ = w.shape[0]
                if need_x:      # dx += dy_g @ w_g : A = dy_g [M, n], B(k = n, j) = w_g[k][j]
                    jobs.append((_p(dy), _p(w), _p(dx), 0, M, K, n_, K, n_, 1, K, 1, 2))
                if ctx.needs_input_grad[1 + 2 * g]:   # dw_g = dy_g^T @ x : A(i = n, k = m) = dy_g[m][i], B(k = m, j) = x[k][j]
                    tgt = _grad_target(w)
                    if tgt is None:
                        gw = torch.empty_like(w)
                    jobs.append((_p(dy), _p(x), _p(tgt if tgt is not None else gw), 0, n_, K, M, K, 1, n_, K, 1, 1 if tgt is not None else 0))
                if b is not None and ctx.needs_input_grad[2 + 2 * g]:
                    tgt = _grad_target(b)
                    if tgt is None:
                        gb = torch.empty_like(b)
                    cjobs.append((_p(dy), 0, _p(tgt if tgt is not None else gb), 0, M, n_, 0, 0, n_, 1, 0, 0, 1 if tgt is not None else 0))
                _note_bgemm(1, M, n_, K, 2)
            grads += [gw, gb]
        if jobs:
            check(lib.gim_bgemm_grouped(*_gemm_tables(jobs, raw=st), st), "bgemm_grouped")
        if cjobs:
            check(lib.gim_colsum_grouped(*_gemm_tables(cjobs, True, st), st), "colsum_grouped")
        return (dx, *grads)


def grouped_linear(x, layers):
    """[y_g] for the (weight, bias) pairs in `layers`, all applied to x [M, K]."""
    flat = []
    for w, b in layers:
        flat += [w, b]
    return GroupedLinearFn.apply(x, *flat)


# --------------------------------------------------------------------------------------------
# instance norm / AdaIN
# --------------------------------------------------------------------------------------------
class NormFn(Function):
    """mode 0: InstanceNorm2d(affine) with scale/shift [C]; mode 1: ada_in with scale/shift [N,C].
    Optional residual added to the output.  x NHWC [N,H,W,C]."""

    @staticmethod
    def forward(ctx, x, scale, shift, res, mode, eps, post_slope=1.0):
        """post_slope != 1: the output is stored ACTIVATED for a conv that is its only reader and runs with x_act (ConvFn): that
        conv's dgrad hands back the gradient w.r.t. the RAW output, so this backward is unchanged (it never reads y)."""
        lib = _lib.load()
        x = _req(x, "x")
        scale_in, shift_in = scale, shift
        scale = _req(scale, "scale")
        shift = _req(shift, "shift")
        N, H, W, C = x.shape
        y = torch.empty_like(x)
        stats = torch.empty((N, C, 3), device=x.device, dtype=torch.float32)
        if res is not None:
            res = _req(res, "res")
        if post_slope != 1.0:
            check(lib.gim_norm_fwd_act(_p(x), _p(scale), _p(shift), _p(res), _p(y), _p(stats), N, H * W, C, mode, eps, post_slope, _stream()), "norm_fwd_act")
        else:
            check(lib.gim_norm_fwd(_p(x), _p(scale), _p(shift), _p(res), _p(y), _p(stats), N, H * W, C, mode, eps, _stream()), "norm_fwd")
        ctx.save_for_backward(x, scale, stats)
        ctx.cfg = (N, H * W, C, mode, res is not None)
        ctx.scale_param, ctx.shift_param = (scale_in, shift_in) if mode == 0 else (None, None)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        lib = _lib.load()
        x, scale, stats = ctx.saved_tensors
        N, HW, C, mode, has_res = ctx.cfg
        dy = _req(dy, "dy")
        st = _stream()
        dx = torch.empty_like(x)
        dsc = torch.empty((N, C), device=x.device, dtype=torch.float32)
        dsh = torch.empty((N, C), device=x.device, dtype=torch.float32)
        check(lib.gim_norm_bwd(_p(dy), _p(x), _p(scale), _p(stats), _p(dx), _p(dsc), _p(dsh), N, HW, C, mode, st), "norm_bwd")
        if mode == 0:
            # affine gradients: one launch, added straight into the parameters' .grad when that is the optimizer's flat
            # bucket (no AccumulateGrad add kernels: 6 launches -> 1 per InstanceNorm layer)
            tgt_s, tgt_b = _grad_target(ctx.scale_param), _grad_target(ctx.shift_param)
            if not (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]):
                dscale = dshift = None
            elif (tgt_s is not None and tgt_b is not None and ctx.needs_input_grad[1] and ctx.needs_input_grad[2]
                  and not torch.is_grad_enabled()):
                check(lib.gim_colsum2(_p(dsc), _p(dsh), _p(tgt_s), _p(tgt_b), N, C, 1, st), "colsum2")
                dscale = dshift = None
            else:
                dscale = torch.empty(C, device=x.device, dtype=torch.float32)
                dshift = torch.empty(C, device=x.device, dtype=torch.float32)
                check(lib.gim_colsum2(_p(dsc), _p(dsh), _p(dscale), _p(dshift), N, C, 0, st), "colsum2")
        else:
            dscale, dshift = dsc.view_as(scale), dsh.view_as(scale)
        return dx, dscale, dshift, (dy if has_res else None), None, None, None


def instance_norm(x, weight, bias, eps=1e-5, post_slope=1.0):
    """post_slope != 1 (and activated storage on): returns lrelu(y) for a conv called with x_act=True - see NormFn.forward."""
    return NormFn.apply(x, weight, bias, None, 0, eps, post_slope if _ACT_STORAGE else 1.0)


def ada_in(x, mean_style, std_style, res=None, eps=1e-5, post_slope=1.0):
    return NormFn.apply(x, std_style, mean_style, res, 1, eps, post_slope if _ACT_STORAGE else 1.0)


def act_storage():
    """Is activated storage in use (ops.conv2d_post_act / norm post_slope + x_act consumers)?  Host-side A/B switch GIM_NO_ACT_STORAGE."""
    return _ACT_STORAGE


# --------------------------------------------------------------------------------------------
# pooling / pointwise
# --------------------------------------------------------------------------------------------
def _avgpool2(x, in_slope):
    """-> (x checked, avgpool2 of the raw x); in_slope != 1: x is stored activated and the kernel inverts that on the fly."""
    lib = _lib.load()
    x = _req(x, "x")
    N, H, W, C = x.shape
    y = torch.empty((N, H // 2, W // 2, C), device=x.device, dtype=torch.float32)
    if in_slope != 1.0:
        check(lib.gim_avgpool2_fwd_act(_p(x), _p(y), N, H, W, C, in_slope, _stream()), "avgpool2_fwd_act")
    else:
        check(lib.gim_avgpool2_fwd(_p(x), _p(y), N, H, W, C, _stream()), "avgpool2_fwd")
    return x, y


class AvgPool2Fn(Function):
    """2x2 average pool.  in_slope != 1: x is stored ACTIVATED (lrelu(x, in_slope) written by its producer for the conv that reads
    it next to this pool); the kernel inverts the activation on the fly.  The gradient handed back is w.r.t. the RAW x - what
    every consumer of an activated tensor returns (ConvFn with x_act) - and does not depend on x: the backward is unchanged."""

    @staticmethod
    def forward(ctx, x, in_slope=1.0):
        x, y = _avgpool2(x, in_slope)
        ctx.cfg = tuple(x.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        return AvgPool2BwdFn.apply(dy, ctx.cfg), None


class AvgPool2BwdFn(Function):
    """dx of the 2x2 average pool (a linear map; its adjoint is the pool itself)."""

    @staticmethod
    def forward(ctx, dy, cfg):
        lib = _lib.load()
        N, H, W, C = cfg
        dy = _req(dy, "dy")
        dx = torch.empty((N, H, W, C), device=dy.device, dtype=torch.float32)
        check(lib.gim_avgpool2_bwd(_p(dy), _p(dx), N, H, W, C, _stream()), "avgpool2_bwd")
        return dx

    @staticmethod
    def backward(ctx, g):
        return AvgPool2Fn.apply(g), None


class ForkFn(Function):
    """n aliases of x for n consumers.  Autograd sums the gradients of a tensor with several consumers pairwise - one launch and one
    full read-modify-write per extra consumer; here each consumer gets an alias of its own and the backward adds all incoming
    gradients in ONE kernel (gim_add_n).  Under create_graph (the R1 term) the sum is built from differentiable additions."""

    @staticmethod
    def forward(ctx, x, n):
        return tuple(x.view_as(x) for _ in range(n))

    @staticmethod
    def backward(ctx, *gs):
        gs = [g for g in gs if g is not None]
        if not gs:
            return None, None
        if len(gs) == 1:
            return gs[0], None
        if _second_order():
            out = gs[0]
            for g in gs[1:]:
                out = out + g
            return out, None
        lib = _lib.load()
        gs = [_req(g, "g") for g in gs]
        out = torch.empty_like(gs[0])
        cur, rest = gs[0], gs[1:]
        while rest:
            take, rest = rest[:3], rest[3:]
            ptrs = [_p(t) for t in take] + [None] * (3 - len(take))
            check(lib.gim_add_n(_p(cur), ptrs[0], ptrs[1], ptrs[2], _p(out), out.numel(), _stream()), "add_n")
            cur = out
        return out, None


def fork(x, n):
    return ForkFn.apply(x, n) if (n > 1 and x.requires_grad and torch.is_grad_enabled()) else (x,) * n


class ForkPoolFn(Function):
    """(alias of x, avgpool2(x)) for the two consumers of a ResBlockDown's input (conv path / pooled skip path); the backward
    adds the conv path's gradient and the un-pooled skip gradient in one kernel (instead of avgpool2_bwd + an autograd addition)."""

    @staticmethod
    def forward(ctx, x, in_slope):
        x, y = _avgpool2(x, in_slope)
        ctx.cfg = tuple(x.shape)
        return x.view_as(x), y

    @staticmethod
    def backward(ctx, g, dyp):
        if dyp is None:
            return g, None
        if g is None or _second_order():
            gp = AvgPool2BwdFn.apply(dyp, ctx.cfg)
            return (gp if g is None else g + gp), None
        lib = _lib.load()
        N, H, W, C = ctx.cfg
        g, dyp = _req(g, "g"), _req(dyp, "dy")
        out = torch.empty_like(g)
        check(lib.gim_add_avgpool2_bwd(_p(g), _p(dyp), _p(out), N, H, W, C, _stream()), "add_avgpool2_bwd")
        return out, None


def fork_pool(x, in_slope=1.0):
    """(x for the conv path, avgpool2(x) for the skip path) - see ForkPoolFn; plain pooling when x carries no gradient."""
    if x.requires_grad and torch.is_grad_enabled():
        return ForkPoolFn.apply(x, in_slope)
    return x, AvgPool2Fn.apply(x, in_slope)


class MaxPoolLreluFn(Function):
    """AdaptiveMaxPool2d((1,1)) -> flatten -> LeakyReLU(0.2) on NHWC input; output [N, C]."""

    @staticmethod
    def forward(ctx, x):
        lib = _lib.load()
        x = _req(x, "x")
        N, H, W, C = x.shape
        y = torch.empty((N, C), device=x.device, dtype=torch.float32)
        idx = torch.empty((N, C), device=x.device, dtype=torch.int32)
        check(lib.gim_maxpool_lrelu_fwd(_p(x), _p(y), idx.data_ptr(), N, H * W, C, LRELU_SLOPE, _stream()), "maxpool_lrelu_fwd")
        ctx.save_for_backward(y, idx)
        ctx.cfg = (N, H, W, C)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, idx = ctx.saved_tensors
        return MaxPoolLreluBwdFn.apply(dy, y.detach(), idx, ctx.cfg)


class MaxPoolLreluBwdFn(Function):
    """dx of MaxPoolLreluFn: routes lrelu'(y) * dy to the arg-max pixel (linear in dy; routing is piecewise constant)."""

    @staticmethod
    def forward(ctx, dy, y, idx, cfg):
        lib = _lib.load()
        N, H, W, C = cfg
        dy = _req(dy, "dy")
        dx = torch.empty((N, H, W, C), device=dy.device, dtype=torch.float32)
        check(lib.gim_maxpool_lrelu_bwd(_p(dy), _p(y), idx.data_ptr(), _p(dx), N, H * W, C, LRELU_SLOPE, _stream()), "maxpool_lrelu_bwd")
        ctx.save_for_backward(y, idx)
        ctx.cfg = cfg
        return dx

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        y, idx = ctx.saved_tensors
        N, H, W, C = ctx.cfg
        g = _req(g, "g")
        gdy = torch.empty((N, C), device=g.device, dtype=torch.float32)
        check(lib.gim_maxpool_gather(_p(g), _p(y), idx.data_ptr(), _p(gdy), N, H * W, C, LRELU_SLOPE, _stream()), "maxpool_gather")
        return gdy, None, None, None


class TanhFn(Function):
    @staticmethod
    def forward(ctx, x):
        lib = _lib.load()
        x = _req(x, "x")
        y = torch.empty_like(x)
        check(lib.gim_tanh_fwd(_p(x), _p(y), x.numel(), _stream()), "tanh_fwd")
        ctx.save_for_backward(y)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        lib = _lib.load()
        (y,) = ctx.saved_tensors
        dy = _req(dy, "dy")
        dx = torch.empty_like(y)
        check(lib.gim_tanh_bwd(_p(dy), _p(y), _p(dx), y.numel(), _stream()), "tanh_bwd")
        return dx


class ScaleAddFn(Function):
    """y = gamma * a + x with gamma a 1-element parameter (SelfAttention output).  post_slope != 1: y is stored activated,
    lrelu(y, post_slope), for consumers that take activated storage (ConvFn x_act, AvgPool2Fn in_slope); they hand back the
    gradient w.r.t. the raw y, and this backward never reads y."""

    @staticmethod
    def forward(ctx, a, x, gamma, post_slope=1.0):
        lib = _lib.load()
        a, x = _req(a, "a"), _req(x, "x")
        y = torch.empty_like(x)
        if post_slope != 1.0:
            check(lib.gim_scale_add_fwd_act(_p(a), _p(x), _p(gamma), _p(y), x.numel(), post_slope, _stream()), "scale_add_fwd_act")
        else:
            check(lib.gim_scale_add_fwd(_p(a), _p(x), _p(gamma), _p(y), x.numel(), _stream()), "scale_add_fwd")
        ctx.save_for_backward(a, gamma)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        a, gamma = ctx.saved_tensors
        dy = _req(dy, "dy")
        if _second_order():
            return (MulScalarFn.apply(dy, gamma) if ctx.needs_input_grad[0] else None), dy, None, None
        da = torch.empty_like(a)
        dg = torch.empty(1, device=dy.device, dtype=torch.float32)
        scratch = torch.empty(2048, device=dy.device, dtype=torch.float32)
        check(lib.gim_scale_add_bwd(_p(dy), _p(a), _p(gamma), _p(da), _p(dg), _p(scratch), a.numel(), _stream()), "scale_add_bwd")
        return da, dy, dg.view_as(gamma), None


class MulScalarFn(Function):
    """y = gamma * x with gamma a 1-element tensor (the attention branch of ScaleAddFn's backward, made differentiable)."""

    @staticmethod
    def forward(ctx, x, gamma):
        y, _ = MulScalarFn._run(x, x, gamma)
        ctx.save_for_backward(x, gamma)
        return y

    @staticmethod
    def _run(dy, a, gamma):
        """(gamma * dy, sum(dy * a)) - one launch of the scale_add backward kernel."""
        lib = _lib.load()
        dy, a = _req(dy, "dy"), _req(a, "a")
        da = torch.empty_like(dy)
        dg = torch.empty(1, device=dy.device, dtype=torch.float32)
        scratch = torch.empty(2048, device=dy.device, dtype=torch.float32)
        check(lib.gim_scale_add_bwd(_p(dy), _p(a), _p(gamma), _p(da), _p(dg), _p(scratch), a.numel(), _stream()), "scale_add_bwd")
        return da, dg

    @staticmethod
    def backward(ctx, g):
        x, gamma = ctx.saved_tensors
        gx, gg = MulScalarFn._run(g, x, gamma)
        return gx, gg.view_as(gamma)


class ToNHWCFn(Function):
    """[N, C, H, W] contiguous -> [N, H, W, C]."""

    @staticmethod
    def forward(ctx, x):
        lib = _lib.load()
        x = _req(x, "x")
        N, C, H, W = x.shape
        ctx.cfg = (N, C, H, W)
        if C == 1:
            return x.view(N, H, W, 1)
        y = torch.empty((N, H, W, C), device=x.device, dtype=torch.float32)
        check(lib.gim_nchw_to_nhwc(_p(x), _p(y), N, C, H * W, _stream()), "nchw_to_nhwc")
        return y

    @staticmethod
    def backward(ctx, dy):
        return ToNCHWFn.apply(dy)


class ToNCHWFn(Function):
    """[N, H, W, C] contiguous -> [N, C, H, W]."""

    @staticmethod
    def forward(ctx, x):
        lib = _lib.load()
        x = _req(x, "x")
        N, H, W, C = x.shape
        ctx.cfg = (N, C, H, W)
        if C == 1:
            return x.view(N, 1, H, W)
        y = torch.empty((N, C, H, W), device=x.device, dtype=torch.float32)
        check(lib.gim_nhwc_to_nchw(_p(x), _p(y), N, C, H * W, _stream()), "nhwc_to_nchw")
        return y

    @staticmethod
    def backward(ctx, dy):
        return ToNHWCFn.apply(dy)


# --------------------------------------------------------------------------------------------
# self-attention core
# --------------------------------------------------------------------------------------------
def _bgemm(A, B, C, batch, M, N, K, sA, sB):
    _note_bgemm(batch, M, N, K)
    check(_lib.load().gim_bgemm(_p(A), _p(B), _p(C), batch, M, N, K, sA[0], sA[1], sA[2], sB[0], sB[1], sB[2], _stream()), "bgemm")


class BgemmFn(Function):
    """C[b] = op(A[b]) @ op(B[b]) for contiguous [batch, rows, cols] operands, op = transpose when tA / tB.
    Bilinear: its backward is two more batched GEMMs, expressed through BgemmFn so that they are differentiable too."""

    @staticmethod
    def forward(ctx, A, B, tA, tB):
        A, B = _req(A, "A"), _req(B, "B")
        nb, ra, ca = A.shape
        _, rb, cb = B.shape
        M, K = (ca, ra) if tA else (ra, ca)
        K2, N = (cb, rb) if tB else (rb, cb)
        if K != K2 or B.shape[0] != nb:
            raise RuntimeError("bgemm: inner dimensions differ (%s %s, tA=%d tB=%d)" % (tuple(A.shape), tuple(B.shape), tA, tB))
        C = torch.empty((nb, M, N), device=A.device, dtype=torch.float32)
        _bgemm(A, B, C, nb, M, N, K, (ra * ca, 1, ca) if tA else (ra * ca, ca, 1), (rb * cb, 1, cb) if tB else (rb * cb, cb, 1))
        ctx.save_for_backward(A, B)
        ctx.t = (tA, tB)
        return C

    @staticmethod
    def backward(ctx, dC):
        A, B = ctx.saved_tensors
        tA, tB = ctx.t
        dA = dB = None
        if ctx.needs_input_grad[0]:
            # C = A op(B): dA = dC op(B)^T ;  C = A^T op(B): dA = op(B) dC^T
            dA = BgemmFn.apply(B, dC, tB, 1) if tA else BgemmFn.apply(dC, B, 0, 1 - tB)
        if ctx.needs_input_grad[1]:
            # C = op(A) B: dB = op(A)^T dC ;  C = op(A) B^T: dB = dC^T op(A)
            dB = BgemmFn.apply(dC, A, 1, tA) if tB else BgemmFn.apply(A, dC, 1 - tA, 0)
        return dA, dB, None, None


class SoftmaxDim1Fn(Function):
    """softmax over dim 1 of [B, R, C] (the reference's attention normalises over the key index, dim -2)."""

    @staticmethod
    def forward(ctx, S):
        S = _req(S, "S")
        Nb, R, C = S.shape
        P = torch.empty_like(S)
        check(_lib.load().gim_softmax_dim1_fwd(_p(S), _p(P), Nb, R, C, _stream()), "softmax_dim1_fwd")
        ctx.save_for_backward(P)
        return P

    @staticmethod
    def backward(ctx, dP):
        (P,) = ctx.saved_tensors
        return SoftmaxDim1BwdFn.apply(dP, P)


class SoftmaxDim1BwdFn(Function):
    """dS = P * (dP - colsum(P * dP)) as an operator of (dP, P)."""

    @staticmethod
    def forward(ctx, dP, P):
        dP, P = _req(dP, "dP"), _req(P, "P")
        Nb, R, C = P.shape
        dS = torch.empty_like(P)
        check(_lib.load().gim_softmax_dim1_bwd(_p(dP), _p(P), _p(dS), Nb, R, C, _stream()), "softmax_dim1_bwd")
        ctx.save_for_backward(dP, P)
        return dS

    @staticmethod
    def backward(ctx, gS):
        lib = _lib.load()
        dP, P = ctx.saved_tensors
        gS = _req(gS, "gS")
        Nb, R, C = P.shape
        g_dP = g_P = None
        if ctx.needs_input_grad[0]:   # the Jacobian w.r.t. dP is symmetric
            g_dP = torch.empty_like(P)
            check(lib.gim_softmax_dim1_bwd(_p(gS), _p(P), _p(g_dP), Nb, R, C, _stream()), "softmax_dim1_bwd")
        if ctx.needs_input_grad[1]:
            g_P = torch.empty_like(P)
            check(lib.gim_softmax_dim1_bwd_dp(_p(gS), _p(dP), _p(P), _p(g_P), Nb, R, C, _stream()), "softmax_dim1_bwd_dp")
        return g_dP, g_P


class AttnProbFn(Function):
    """A[b] = softmax over dim 1 of f[b] g[b]^T in ONE kernel (gim_attn_prob_fwd: the T x T energy never goes through memory) for
    the shape the benchmark networks use (T = 256 tokens, C/8 = 16 channels).  Its backward is the unfused one, expressed through
    SoftmaxDim1BwdFn and BgemmFn so that it stays differentiable (the R1 term differentiates the discriminator's attention twice)."""

    @staticmethod
    def supported(f, g):
        return f.dim() == 3 and f.shape[1] == 256 and f.shape[2] == 16 and g.shape == f.shape

    @staticmethod
    def forward(ctx, f, g):
        f, g = _req(f, "f"), _req(g, "g")
        nb, T, K = f.shape
        A = torch.empty((nb, T, T), device=f.device, dtype=torch.float32)
        _note_bgemm(nb, T, T, K)
        check(_lib.load().gim_attn_prob_fwd(_p(f), _p(g), _p(A), nb, T, K, _stream()), "attn_prob_fwd")
        ctx.save_for_backward(f, g, A)
        return A

    @staticmethod
    def backward(ctx, dA):
        f, g, A = ctx.saved_tensors
        dS = SoftmaxDim1BwdFn.apply(dA, A)
        df = BgemmFn.apply(dS, g, 0, 0) if ctx.needs_input_grad[0] else None     # S = f g^T: dS g
        dg = BgemmFn.apply(dS, f, 1, 0) if ctx.needs_input_grad[1] else None     #            dS^T f
        return df, dg


def attn_core(f, g, h):
    """out[b, j, :] = sum_i softmax_i(f[b,i,:] . g[b,j,:]) * h[b,i,:]   (tokens = pixels, NHWC rows)."""
    if _FUSED_ATTN and AttnProbFn.supported(f, g):
        A = AttnProbFn.apply(f, g)
    else:
        S = BgemmFn.apply(f, g, 0, 1)        # S[i, j] = f_i . g_j
        A = SoftmaxDim1Fn.apply(S)
    return BgemmFn.apply(A, h, 1, 0)     # out = A^T h


_FUSED_ATTN = os.environ.get("GIM_NO_FUSED_ATTN") is None   # A/B switch (host side)


# --------------------------------------------------------------------------------------------
# set pooling (authenticator head) and small glue of the generator
# --------------------------------------------------------------------------------------------
class SumDim1Fn(Function):
    """y[b] = scale * sum_j x[b, j]  for x [B, t, D]."""

    @staticmethod
    def forward(ctx, x, scale):
        lib = _lib.load()
        x = _req(x, "x")
        B, t, D = x.shape
        y = torch.empty((B, D), device=x.device, dtype=torch.float32)
        check(lib.gim_sum_dim1(_p(x), _p(y), B, t, D, scale, _stream()), "sum_dim1")
        ctx.cfg = (B, t, D, scale)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        lib = _lib.load()
        B, t, D, scale = ctx.cfg
        dy = _req(dy, "dy")
        dx = torch.empty((B, t, D), device=dy.device, dtype=torch.float32)
        check(lib.gim_repeat_dim1(_p(dy), _p(dx), B, t, D, scale, _stream()), "repeat_dim1")
        return dx, None


class RepeatDim1Fn(Function):
    """y[b, j] = x[b] for j < t: [B, D] -> [B, t, D]."""

    @staticmethod
    def forward(ctx, x, t):
        lib = _lib.load()
        x = _req(x, "x")
        B, D = x.shape
        y = torch.empty((B, t, D), device=x.device, dtype=torch.float32)
        check(lib.gim_repeat_dim1(_p(x), _p(y), B, t, D, 1.0, _stream()), "repeat_dim1")
        ctx.cfg = (B, t, D)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        lib = _lib.load()
        B, t, D = ctx.cfg
        dy = _req(dy, "dy")
        dx = torch.empty((B, D), device=dy.device, dtype=torch.float32)
        check(lib.gim_sum_dim1(_p(dy), _p(dx), B, t, D, 1.0, _stream()), "sum_dim1")
        return dx, None


def mean_dim1(x):
    return SumDim1Fn.apply(x, 1.0 / x.shape[1])


class NoiseCombineFn(Function):
    """noisy[b, j] = env[b] + w[b, j] - mean_j w[b, j]  (mean term iff remove_mean)."""

    @staticmethod
    def forward(ctx, env, w, remove_mean):
        lib = _lib.load()
        env, w = _req(env, "env"), _req(w, "w")
        B, t, D = w.shape
        y = torch.empty_like(w)
        check(lib.gim_noise_combine(_p(env), _p(w), _p(y), B, t, D, 1 if remove_mean else 0, _stream()), "noise_combine")
        ctx.cfg = (B, t, D, remove_mean)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        lib = _lib.load()
        B, t, D, remove_mean = ctx.cfg
        dy = _req(dy, "dy")
        denv = torch.empty((B, D), device=dy.device, dtype=torch.float32)
        check(lib.gim_sum_dim1(_p(dy), _p(denv), B, t, D, 1.0, _stream()), "sum_dim1")
        dw = torch.empty_like(dy)
        check(lib.gim_noise_combine(None, _p(dy), _p(dw), B, t, D, 1 if remove_mean else 0, _stream()), "noise_combine")
        return denv, dw, None


class Concat2Fn(Function):
    """cat((a, b broadcast), channel) for NHWC a [R_img, H, W, Ca] and b [R_img/rep, H, W, Cb]
    (each b image serves `rep` consecutive a images).  Gradient flows to a only."""

    @staticmethod
    def forward(ctx, a, b, rep):
        lib = _lib.load()
        a, b = _req(a, "a"), _req(b, "b")
        Ni, H, W, Ca = a.shape
        Cb = b.shape[3]
        y = torch.empty((Ni, H, W, Ca + Cb), device=a.device, dtype=torch.float32)
        check(lib.gim_concat2(_p(a), _p(b), _p(y), Ni * H * W, Ca, Cb, H * W, rep, _stream()), "concat2")
        ctx.cfg = (Ni, H, W, Ca, Cb)
        ctx.rep = rep
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        lib = _lib.load()
        Ni, H, W, Ca, Cb = ctx.cfg
        dy = _req(dy, "dy")
        da = db = None
        if ctx.needs_input_grad[0]:
            da = torch.empty((Ni, H, W, Ca), device=dy.device, dtype=torch.float32)
            check(lib.gim_slice_channels(_p(dy), _p(da), Ni * H * W, Ca, Ca + Cb, _stream()), "slice_channels")
        if ctx.needs_input_grad[1]:
            if ctx.rep != 1:
                raise RuntimeError("concat2: gradient w.r.t. a broadcast second operand is not implemented")
            db = torch.empty((Ni, H, W, Cb), device=dy.device, dtype=torch.float32)
            check(lib.gim_slice_channels(_p(dy, Ca), _p(db), Ni * H * W, Cb, Ca + Cb, _stream()), "slice_channels")
        return da, db, None


class HeadCatFn(Function):
    """The [B, 2*(Ds + 2*De + Df)] input of the authenticator's MLP:
    cat(mean(test_src), mean(si_src), [mean, custom_std](test_env), mean(fc_test), [mean, custom_std](si_env), mean(fc_si))
    where fc_* are the per-sample outputs of the FC-stat MLP."""

    @staticmethod
    def forward(ctx, test_src, test_env, si_src, si_env, fc_test, fc_si):
        lib = _lib.load()
        ts, te, ss, se, ft, fs = [_req(t, "head input") for t in (test_src, test_env, si_src, si_env, fc_test, fc_si)]
        B, n, Ds = ts.shape
        k = ss.shape[1]
        De, Df = te.shape[2], ft.shape[2]
        L = 2 * (Ds + 2 * De + Df)
        out = torch.empty((B, L), device=ts.device, dtype=torch.float32)
        st = _stream()
        o_te = 2 * Ds
        o_se = o_te + 2 * De + Df
        check(lib.gim_set_stats_fwd(_p(ts), _p(out, 0), None, B, n, Ds, L, L, st), "set_stats_fwd")
        check(lib.gim_set_stats_fwd(_p(ss), _p(out, Ds), None, B, k, Ds, L, L, st), "set_stats_fwd")
        check(lib.gim_set_stats_fwd(_p(te), _p(out, o_te), _p(out, o_te + De), B, n, De, L, L, st), "set_stats_fwd")
        check(lib.gim_set_stats_fwd(_p(ft), _p(out, o_te + 2 * De), None, B, n, Df, L, L, st), "set_stats_fwd")
        check(lib.gim_set_stats_fwd(_p(se), _p(out, o_se), _p(out, o_se + De), B, k, De, L, L, st), "set_stats_fwd")
        check(lib.gim_set_stats_fwd(_p(fs), _p(out, o_se + 2 * De), None, B, k, Df, L, L, st), "set_stats_fwd")
        ctx.save_for_backward(ts, te, ss, se, ft, fs)
        return out

    @staticmethod
    def backward(ctx, dout):
        ts, te, ss, se, ft, fs = ctx.saved_tensors
        dout = _req(dout, "dout")
        Ds, De, Df = ts.shape[2], te.shape[2], ft.shape[2]
        o_te = 2 * Ds
        o_se = o_te + 2 * De + Df
        second = _second_order()
        slots = ((ts, 0, None), (te, o_te, o_te + De), (ss, Ds, None), (se, o_se, o_se + De), (ft, o_te + 2 * De, None), (fs, o_se + 2 * De, None))
        return tuple(_set_stats_bwd(dout, x, o_mean, o_std, second) if need else None
                     for (x, o_mean, o_std), need in zip(slots, ctx.needs_input_grad))


class StatCatFn(Function):
    """cat(mean(x, 1), custom_std(x), mean(fc, 1)) for x [B, t, D] and the per-sample FC features fc [B, t, Df] -> [B, 2 D + Df]
    (GIMMeanStdFcStat.forward, models/gim_basic_models.py:152-172, as a standalone operator; the authenticator head uses the
    two-set form HeadCatFn)."""

    @staticmethod
    def forward(ctx, x, fc):
        lib = _lib.load()
        x, fc = _req(x, "x"), _req(fc, "fc")
        B, t, D = x.shape
        Df = fc.shape[2]
        L = 2 * D + Df
        out = torch.empty((B, L), device=x.device, dtype=torch.float32)
        st = _stream()
        check(lib.gim_set_stats_fwd(_p(x), _p(out, 0), _p(out, D), B, t, D, L, L, st), "set_stats_fwd")
        check(lib.gim_set_stats_fwd(_p(fc), _p(out, 2 * D), None, B, t, Df, L, L, st), "set_stats_fwd")
        ctx.save_for_backward(x, fc)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, fc = ctx.saved_tensors
        dout = _req(dout, "dout")
        D = x.shape[2]
        second = _second_order()
        return tuple(_set_stats_bwd(dout, src, o_mean, o_std, second) if need else None
                     for (src, o_mean, o_std), need in zip(((x, 0, D), (fc, 2 * D, None)), ctx.needs_input_grad))


stat_cat = StatCatFn.apply


def _set_stats_bwd(dout, x, o_mean, o_std, second):
    """Gradient w.r.t. x [B, t, D] of one mean (o_std None) / [mean, custom_std] slot at columns o_mean / o_std of the row dout
    [B, L] (gim_set_stats_bwd); second: as the differentiable operator SetStatsBwdFn (R1)."""
    if second:
        return SetStatsBwdFn.apply(dout, x, o_mean, o_std)
    B, t, D = x.shape
    L = dout.shape[1]
    dx = torch.empty_like(x)
    check(_lib.load().gim_set_stats_bwd(_p(x), _p(dout, o_mean), (_p(dout, o_std) if o_std is not None else None), _p(dx),
                                        B, t, D, L, L, _stream()), "set_stats_bwd")
    return dx


class SetStatsBwdFn(Function):
    """dx[b, j] = dout[b, o_mean:] / t + dout[b, o_std:] * (x[b, j] - mean) / ((t - 1) * custom_std)  as an operator of (dout, x):
    the backward of one mean / [mean, custom_std] slot of the authenticator head, differentiable for the R1 term."""

    @staticmethod
    def forward(ctx, dout, x, o_mean, o_std):
        dout, x = _req(dout, "dout"), _req(x, "x")
        dx = _set_stats_bwd(dout, x, o_mean, o_std, False)
        ctx.save_for_backward(dout, x)
        ctx.o = (o_mean, o_std)
        return dx

    @staticmethod
    def backward(ctx, g):
        dout, x = ctx.saved_tensors
        o_mean, o_std = ctx.o
        g = _req(g, "g")
        B, t, D = x.shape
        L = dout.shape[1]
        g_dout = torch.zeros_like(dout) if ctx.needs_input_grad[0] else None
        gx = torch.empty_like(x) if (ctx.needs_input_grad[1] and o_std is not None) else None
        check(_lib.load().gim_set_stats_bwd_bwd(_p(x), (_p(dout, o_std) if o_std is not None else None), _p(g),
                                                (_p(g_dout, o_mean) if g_dout is not None else None),
                                                (_p(g_dout, o_std) if (g_dout is not None and o_std is not None) else None),
                                                _p(gx), B, t, D, L, L, _stream()), "set_stats_bwd_bwd")
        return g_dout, gx, None, None


class SqSumRowsFn(Function):
    """out[b] = sum_i x[b, i]^2  (the g.pow(2).view(B, -1).sum(1) of compute_grad2, training/utils.py:122)."""

    @staticmethod
    def forward(ctx, x):
        x = _req(x, "x")
        B, L = x.shape
        out = torch.empty(B, device=x.device, dtype=torch.float32)
        check(_lib.load().gim_sqsum_rows_fwd(_p(x), _p(out), B, L, _stream()), "sqsum_rows_fwd")
        ctx.save_for_backward(x)
        return out

    @staticmethod
    def backward(ctx, dout):
        (x,) = ctx.saved_tensors
        if torch.is_grad_enabled():
            raise NotImplementedError("third-order gradients are not supported")
        dout = _req(dout, "dout")
        B, L = x.shape
        dx = torch.empty_like(x)
        check(_lib.load().gim_sqsum_rows_bwd(_p(x), _p(dout), _p(dx), B, L, _stream()), "sqsum_rows_bwd")
        return dx


sqsum_rows = SqSumRowsFn.apply


class BCELogitsFn(Function):
    """binary_cross_entropy_with_logits(x, full_like(x, target), reduction='none')."""

    @staticmethod
    def forward(ctx, x, target):
        lib = _lib.load()
        x = _req(x, "x")
        loss = torch.empty_like(x)
        check(lib.gim_bce_logits_fwd(_p(x), _p(loss), target, x.numel(), _stream()), "bce_logits_fwd")
        ctx.save_for_backward(x)
        ctx.target = target
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, dl):
        lib = _lib.load()
        (x,) = ctx.saved_tensors
        dl = _req(dl, "dloss")
        dx = torch.empty_like(x)
        check(lib.gim_bce_logits_bwd(_p(dl), _p(x), _p(dx), ctx.target, x.numel(), _stream()), "bce_logits_bwd")
        return dx, None


avg_pool2 = AvgPool2Fn.apply
maxpool_lrelu = MaxPoolLreluFn.apply
tanh = TanhFn.apply
scale_add = ScaleAddFn.apply
to_nhwc = ToNHWCFn.apply
to_nchw = ToNCHWFn.apply
noise_combine = NoiseCombineFn.apply
concat2 = Concat2Fn.apply
head_cat = HeadCatFn.apply
bce_logits = BCELogitsFn.apply


def repeat_dim1(x, t):
    return RepeatDim1Fn.apply(x, t)


class MeanStdCatFn(Function):
    """cat([mean(x_i, 1), custom_std(x_i)] for each x_i [B, t_i, D]) -> [B, 2*D*len(xs)]
    (GIMMeanStdStat of both sample sets + torch.cat, models/gim_gaussian_models.py:37-39)."""

    @staticmethod
    def forward(ctx, *xs):
        lib = _lib.load()
        xs = [_req(x, "x") for x in xs]
        B, _, D = xs[0].shape
        L = 2 * D * len(xs)
        out = torch.empty((B, L), device=xs[0].device, dtype=torch.float32)
        st = _stream()
        for i, x in enumerate(xs):
            check(lib.gim_set_stats_fwd(_p(x), _p(out, 2 * D * i), _p(out, 2 * D * i + D), B, x.shape[1], D, L, L, st), "set_stats_fwd")
        ctx.save_for_backward(*xs)
        return out

    @staticmethod
    def backward(ctx, dout):
        xs = ctx.saved_tensors
        dout = _req(dout, "dout")
        D = xs[0].shape[2]
        second = _second_order()
        return tuple(_set_stats_bwd(dout, x, 2 * D * i, 2 * D * i + D, second) if ctx.needs_input_grad[i] else None
                     for i, x in enumerate(xs))


def mean_std_cat(*xs):
    return MeanStdCatFn.apply(*xs)


class ImgAttMixFn(Function):
    """out = x1 * a1 + v2 * a2 with (a1, a2) = softmax(sum_c q1*k1, sum_c q2*k2)  (ImgAttention, NHWC)."""

    @staticmethod
    def forward(ctx, q1, k1, q2, k2, x1, v2):
        lib = _lib.load()
        ts = [_req(t, "img_att input") for t in (q1, k1, q2, k2, x1, v2)]
        N, H, W, C = ts[0].shape
        out = torch.empty_like(ts[0])
        att = torch.empty((N, H, W), device=out.device, dtype=torch.float32)
        check(lib.gim_img_att_mix_fwd(*[_p(t) for t in ts], _p(out), _p(att), N * H * W, C, _stream()), "img_att_mix_fwd")
        ctx.save_for_backward(*ts, att)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        lib = _lib.load()
        q1, k1, q2, k2, x1, v2, att = ctx.saved_tensors
        dout = _req(dout, "dout")
        N, H, W, C = q1.shape
        gs = [torch.empty_like(q1) for _ in range(6)]
        check(lib.gim_img_att_mix_bwd(_p(dout), _p(q1), _p(k1), _p(q2), _p(k2), _p(x1), _p(v2), _p(att), *[_p(g) for g in gs],
                                      N * H * W, C, _stream()), "img_att_mix_bwd")
        return tuple(gs)


img_att_mix = ImgAttMixFn.apply


# --------------------------------------------------------------------------------------------
# inference-only operators of the baseline authenticators (baselines.py): no autograd
# --------------------------------------------------------------------------------------------
def _no_grad_inputs(what, *ts):
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts):
        raise RuntimeError("ops.%s is an inference operator (no backward): call it under torch.no_grad()" % what)


def conv2d_infer(x, w, bias=None, slope=None, stride=1):
    """y = prelu_c(conv(x, w, stride, padding=(KH-1)/2) + bias).  x [N, H, W, Cin] NHWC, w [Cout, KH, KH, Cin] (the library's storage
    order), bias / slope [Cout] or None (slope None: no activation, zeros: ReLU).  Returns [N, H/stride, W/stride, Cout]."""
    lib = _lib.load()
    _no_grad_inputs("conv2d_infer", x, w, bias, slope)
    x, w = _req(x, "x"), _req(w, "w")
    N, H, W, Cin = x.shape
    Cout, KH = w.shape[0], w.shape[1]
    if tuple(w.shape) != (Cout, KH, KH, Cin):
        raise RuntimeError("conv2d_infer: weight %s does not match [Cout, KH, KH, Cin = %d]" % (tuple(w.shape), Cin))
    for name, v in (("bias", bias), ("slope", slope)):
        if v is not None and tuple(_req(v, name).shape) != (Cout,):
            raise RuntimeError("conv2d_infer: %s must be [Cout]" % name)
    bias = None if bias is None else _req(bias, "bias")
    slope = None if slope is None else _req(slope, "slope")
    sh = _lib.GimInferConv(N, H, W, Cin, Cout, KH, stride)
    y = torch.empty((N, H // stride, W // stride, Cout), device=x.device, dtype=torch.float32)
    if _FLOPS is not None:
        key = ("infer", (N, H // stride, W // stride, Cin, Cout, KH, stride))
        _FLOPS.setdefault(key, [0, 2.0 * N * (H // stride) * (W // stride) * Cin * Cout * KH * KH])[0] += 1
    check(lib.gim_conv2d_infer(_p(x), _p(w), _p(bias), _p(slope), _p(y), ctypes.byref(sh), _stream()), "conv2d_infer")
    return y


def linear_infer(x, w, bias=None, slope=None):
    """[rows, in] x [out, in]^T (+ bias, + per-output PReLU): conv2d_infer on a 1x1 map."""
    return conv2d_infer(x.view(x.shape[0], 1, 1, x.shape[1]), w.view(w.shape[0], 1, 1, w.shape[1]), bias, slope).view(x.shape[0], w.shape[0])


def maxpool2(x, relu=False):
    """nn.MaxPool2d(2) of an NHWC map; relu: max(., 0) on the pooled value (= pooling the ReLU of the map)."""
    lib = _lib.load()
    _no_grad_inputs("maxpool2", x)
    x = _req(x, "x")
    N, H, W, C = x.shape
    y = torch.empty((N, H // 2, W // 2, C), device=x.device, dtype=torch.float32)
    check(lib.gim_maxpool2_act(_p(x), _p(y), N, H, W, C, 1 if relu else 0, _stream()), "maxpool2_act")
    return y


def channel_affine(x, scale, shift):
    """y = x * scale[c] + shift[c] over the last dim (inference BatchNorm)."""
    lib = _lib.load()
    _no_grad_inputs("channel_affine", x, scale, shift)
    x, scale, shift = _req(x, "x"), _req(scale, "scale"), _req(shift, "shift")
    C = x.shape[-1]
    y = torch.empty_like(x)
    check(lib.gim_channel_affine(_p(x), _p(scale), _p(shift), _p(y), x.numel() // C, C, _stream()), "channel_affine")
    return y


def _se_tail_fwd(what, res, gate, shortcut, sstride, scale=None, shift=None):
    """Checks and forward launch of ops.se_tail / ops.se_tail_train -> (res, gate, out, out_bn or None)."""
    lib = _lib.load()
    res, gate, shortcut = _req(res, "res"), _req(gate, "gate"), _req(shortcut, "shortcut")
    N, Ho, Wo, C = res.shape
    if tuple(shortcut.shape) != (N, Ho * sstride, Wo * sstride, C) or tuple(gate.shape) != (N, C):
        raise RuntimeError("%s: shortcut %s / gate %s do not match res %s at sstride %s"
                           % (what, tuple(shortcut.shape), tuple(gate.shape), tuple(res.shape), sstride))
    out = torch.empty_like(res)
    out_bn = None
    if scale is not None:
        scale, shift = _req(scale, "scale"), _req(shift, "shift")
        out_bn = torch.empty_like(res)
    check(lib.gim_se_tail(_p(res), _p(gate), _p(shortcut), _p(scale), _p(shift), _p(out), _p(out_bn), N, Ho, Wo, C, sstride, _stream()),
          "se_tail")
    return res, gate, out, out_bn


def se_tail(res, gate, shortcut, sstride=1, scale=None, shift=None):
    """out = res * sigmoid(gate[n, c]) + shortcut[n, ::sstride, ::sstride, c]; with scale / shift also out * scale[c] + shift[c].
    Returns out, or (out, out_bn)."""
    _no_grad_inputs("se_tail", res, gate, shortcut, scale, shift)
    _, _, out, out_bn = _se_tail_fwd("se_tail", res, gate, shortcut, sstride, scale, shift)
    return out if out_bn is None else (out, out_bn)


def pair_score(a, b):
    """-(|| a / |a| - b / |b| ||^2) per row of two [B, D] matrices."""
    lib = _lib.load()
    _no_grad_inputs("pair_score", a, b)
    a, b = _req(a, "a"), _req(b, "b")
    if a.shape != b.shape or a.dim() != 2:
        raise RuntimeError("pair_score: two [B, D] matrices of one shape")
    out = torch.empty((a.shape[0],), device=a.device, dtype=torch.float32)
    check(lib.gim_pair_score(_p(a), _p(b), _p(out), a.shape[0], a.shape[1], _stream()), "pair_score")
    return out


def _absdiff_fwd(what, a, b):
    """Checks and forward launch of ops.absdiff / ops.absdiff_train -> (a, b, y)."""
    a, b = _req(a, "a"), _req(b, "b")
    if a.shape != b.shape:
        raise RuntimeError("%s: shapes differ" % what)
    y = torch.empty_like(a)
    check(_lib.load().gim_absdiff(_p(a), _p(b), _p(y), a.numel(), _stream()), "absdiff")
    return a, b, y


def absdiff(a, b):
    """|a - b|, elementwise."""
    _no_grad_inputs("absdiff", a, b)
    return _absdiff_fwd("absdiff", a, b)[2]


def _l2norm_rows_fwd(x):
    """Forward launch of ops.l2norm_rows / ops.l2norm_rows_train -> (x, y)."""
    x = _req(x, "x")
    y = torch.empty_like(x)
    check(_lib.load().gim_l2norm_rows(_p(x), _p(y), x.shape[0], x.shape[1], _stream()), "l2norm_rows")
    return x, y


def l2norm_rows(x):
    """x / |x| per row of a [B, D] matrix."""
    _no_grad_inputs("l2norm_rows", x)
    return _l2norm_rows_fwd(x)[1]


# --------------------------------------------------------------------------------------------
# training the siamese baseline (baseline_training.py): BatchNorm with batch statistics + ReLU + MaxPool2d(2), |a - b|
# --------------------------------------------------------------------------------------------
def bn_slabs(rows):
    """Number of row slabs the two-stage sums of the BatchNorm kernels cut a map of `rows` rows into."""
    n = _lib.load().gim_bn_slabs(rows)
    if n <= 0:
        check(n, "bn_slabs")
    return n


def _slab_partials(rows, C, sums, device):
    """Stage-1 buffer of `sums` per-channel sums over `rows` rows (csrc/rowsum.h): one float per sum, slab and channel."""
    return torch.empty(sums * bn_slabs(rows) * C, device=device, dtype=torch.float32)


def _channel_grads(need, params, sums):
    """The rule for the gradients of per-channel parameters.  need[i]: autograd wants the gradient of params[i] (a [C] tensor or
    None), whose total the kernel writes to sums[i].  -> (acc, grads): acc[i] is the parameter's .grad where that is the optimizer's
    bucket - the kernel ADDS the total there and grads[i] is None - and otherwise None, and grads[i] = sums[i] goes back to autograd."""
    acc = [_grad_target(p) if (p is not None and n) else None for p, n in zip(params, need)]
    grads = [sums[i] if (p is not None and n and acc[i] is None) else None for i, (p, n) in enumerate(zip(params, need))]
    return acc, grads


def _req_map(z, what):
    z = _req(z, what)
    if z.dim() != 4 or z.shape[3] % 4 or z.shape[1] % 2 or z.shape[2] % 2:
        raise RuntimeError("%s must be an NHWC map [N, H, W, C] with H, W even and C %% 4 == 0, got %s" % (what, tuple(z.shape)))
    return z


def _req_rows(x, what):
    """x [..., C] with C % 4 == 0, contiguous -> (x, rows, C)."""
    x = _req(x, what)
    C = x.shape[-1]
    if x.dim() < 2 or C % 4:
        raise RuntimeError("%s must be [..., C] with C %% 4 == 0, got %s" % (what, tuple(x.shape)))
    return x, x.numel() // C, C


def _req_running(what, C, running_mean, running_var, num_batches_tracked, momentum):
    if momentum is None:
        raise NotImplementedError("%s: momentum=None (cumulative moving average) is not implemented" % what)
    for name, v in (("running_mean", running_mean), ("running_var", running_var)):
        if v is not None and (tuple(_req(v, name).shape) != (C,) or not v.is_contiguous()):
            raise RuntimeError("%s: %s must be a contiguous [C] tensor" % (what, name))
    if num_batches_tracked is not None and not (num_batches_tracked.is_cuda and num_batches_tracked.dtype == torch.int64):
        raise RuntimeError("%s: num_batches_tracked must be a CUDA int64 tensor" % what)
    return None if num_batches_tracked is None else num_batches_tracked.data_ptr()


def bn_stats(z, eps=1e-5, running_mean=None, running_var=None, num_batches_tracked=None, momentum=0.1):
    """(mean [C], invstd [C]) over the M >= 2 rows of any [..., C] tensor with C % 4 == 0 (an NHWC map of any size, [B, C] of a
    BatchNorm1d): the biased variance, as nn.BatchNorm normalises in training mode; with running_mean / running_var /
    num_batches_tracked these are updated in place as nn.BatchNorm does (unbiased variance)."""
    lib = _lib.load()
    z, M, C = _req_rows(z, "z")
    if M < 2:
        raise RuntimeError("batch statistics need at least two rows, got %s" % (tuple(z.shape),))
    nbt = _req_running("bn_stats", C, running_mean, running_var, num_batches_tracked, momentum)
    stats = torch.empty((2, C), device=z.device, dtype=torch.float32)
    partials = _slab_partials(M, C, 2, z.device)      # (mean, M2) per slab and channel
    check(lib.gim_bn_stats(_p(z), _p(partials), _p(stats), _p(stats, C), _p(running_mean), _p(running_var), nbt, M, C,
                           float(momentum), float(eps), _stream()), "bn_stats")
    return stats[0], stats[1]


# Data-parallel training: BatchNorm is the one operator of the baselines that couples the images of a batch.  A rank computes the
# record of its rows (bn_stats_record), the ranks' records are gathered and every rank merges them in rank order (bn_stats_merge):
# the same bits everywhere, so the replicas' running statistics stay equal without a broadcast.  In the backward the two per-channel
# sums that enter dz are all-reduced and dz takes 1 / (all ranks' rows); the PARAMETER gradients stay the local sums - the optimizer's
# bucket is all-reduced once more in FusedAdam.step.
BN_MAX_RANKS = 64      # the merge kernel's limit (csrc/bn_train.hip)


def bn_stats_record(z):
    """One rank's share of the batch statistics: [2, C] = (mean, M2 = sum of squared deviations from that mean) over the M >= 1 rows
    of z [..., C], C % 4 == 0."""
    z, M, C = _req_rows(z, "z")
    record = torch.empty((2, C), device=z.device, dtype=torch.float32)
    partials = _slab_partials(M, C, 2, z.device)
    check(_lib.load().gim_bn_stats_record(_p(z), _p(partials), _p(record), M, C, _stream()), "bn_stats_record")
    return record


def bn_stats_merge(records, counts, eps, running_mean=None, running_var=None, num_batches_tracked=None, momentum=0.1):
    """(mean [C], invstd [C]) of the rows behind records [R, 2, C] (bn_stats_record of R <= 64 ranks, in rank order; counts: their
    row counts, host integers >= 1 that sum to >= 2), combined in rank order with Chan's formula and finished as bn_stats finishes:
    the running statistics move with the unbiased variance over all rows.  R = 1 gives the bits of bn_stats."""
    records = _req(records, "records")
    if records.dim() != 3 or records.shape[1] != 2 or records.shape[2] % 4:
        raise RuntimeError("bn_stats_merge: records must be [R, 2, C] with C %% 4 == 0, got %s" % (tuple(records.shape),))
    R, _, C = records.shape
    counts = [int(n) for n in counts]
    if len(counts) != R:
        raise RuntimeError("bn_stats_merge: %d records but %d row counts" % (R, len(counts)))
    nbt = _req_running("bn_stats_merge", C, running_mean, running_var, num_batches_tracked, momentum)
    stats = torch.empty((2, C), device=records.device, dtype=torch.float32)
    check(_lib.load().gim_bn_stats_merge(_p(records), (ctypes.c_int64 * R)(*counts), R, C, _p(stats), _p(stats, C), _p(running_mean),
                                         _p(running_var), nbt, float(momentum), float(eps), _stream()), "bn_stats_merge")
    return stats[0], stats[1]


class DistSync:
    """The `sync` of batch_norm / bn_relu_maxpool2 over torch.distributed (group: a process group, None for the default one).
    What a sync is: `rank`, `world`, all_gather(t) -> [world, *t.shape] in rank order, all_reduce_(t) (sum, in place)."""

    def __init__(self, group=None):
        import torch.distributed as dist
        self._dist, self.group = dist, group
        self.rank, self.world = dist.get_rank(group), dist.get_world_size(group)

    def all_gather(self, t):
        out = torch.empty((self.world,) + tuple(t.shape), device=t.device, dtype=t.dtype)
        self._dist.all_gather(list(out.unbind(0)), t, group=self.group)
        return out

    def all_reduce_(self, t):
        self._dist.all_reduce(t, op=self._dist.ReduceOp.SUM, group=self.group)
        return t


def default_sync():
    """A DistSync when torch.distributed is initialised with more than one rank, else None (the single-process path)."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        return DistSync()
    return None


def _synced(sync):
    return sync is not None and sync.world > 1


def _batch_stats(z, sync, eps, running_mean, running_var, num_batches_tracked, momentum):
    """(mean, invstd) of the whole batch, of which z is this rank's equal share; without a sync z is the whole batch (bn_stats)."""
    if not _synced(sync):
        return bn_stats(z, eps, running_mean, running_var, num_batches_tracked, momentum)
    if sync.world > BN_MAX_RANKS:
        raise RuntimeError("batch statistics are merged over at most %d ranks, got %d" % (BN_MAX_RANKS, sync.world))
    rows = z.numel() // z.shape[-1]
    records = sync.all_gather(bn_stats_record(z))
    return bn_stats_merge(records, [rows] * sync.world, eps, running_mean, running_var, num_batches_tracked, momentum)


def _total_sums(sums, sync):
    """The (dgamma, dbeta) that enter dz: all ranks' sums.  `sums` itself stays local - it is what the parameters receive."""
    return sync.all_reduce_(sums[:2].clone()) if _synced(sync) else sums


def bn_pool_fwd(z, weight, bias, mean, invstd):
    """maxpool2(relu((z - mean) * invstd * weight + bias)) of an NHWC map with GIVEN statistics; no autograd."""
    N, H, W, C = z.shape
    p = torch.empty((N, H // 2, W // 2, C), device=z.device, dtype=torch.float32)
    check(_lib.load().gim_bn_relu_maxpool2_fwd(_p(z), _p(weight), _p(bias), _p(mean), _p(invstd), _p(p), N, H, W, C, _stream()),
          "bn_relu_maxpool2_fwd")
    return p


def bn_pool_bwd_sums(dp, z, weight, bias, mean, invstd, acc=(None, None), out=None):
    """[2, C] = (dgamma, dbeta) of bn_pool_fwd over THIS map's rows (written to `out` where given); acc: (weight.grad, bias.grad)
    buffers the sums are also ADDED to."""
    N, H, W, C = z.shape
    sums = torch.empty((2, C), device=z.device, dtype=torch.float32) if out is None else out
    partials = _slab_partials(N * (H // 2) * (W // 2), C, 2, z.device)
    check(_lib.load().gim_bn_pool_bwd_reduce(_p(dp), _p(z), _p(weight), _p(bias), _p(mean), _p(invstd), _p(partials), _p(sums),
                                             _p(sums, C), _p(acc[0]), _p(acc[1]), N, H, W, C, _stream()), "bn_pool_bwd_reduce")
    return sums


def bn_pool_bwd_dx(dp, z, weight, bias, mean, invstd, sums, total_rows=None):
    """dz of bn_pool_fwd from sums = (dgamma, dbeta).  total_rows: the pre-pool rows of ALL ranks when sums are all ranks' totals
    (None: this map's own N * H * W rows)."""
    lib = _lib.load()
    N, H, W, C = z.shape
    dz = torch.empty_like(z)
    args = (_p(dp), _p(z), _p(weight), _p(bias), _p(mean), _p(invstd), _p(sums), _p(sums, C), _p(dz), N, H, W, C)
    if total_rows is None:
        check(lib.gim_bn_pool_bwd_dx(*args, _stream()), "bn_pool_bwd_dx")
    else:
        check(lib.gim_bn_pool_bwd_dx_total(*args, int(total_rows), _stream()), "bn_pool_bwd_dx_total")
    return dz


class BnReluMaxPool2Fn(Function):
    """p = maxpool2(relu(batch_norm(z))) with BATCH statistics: nn.BatchNorm2d in training mode -> nn.ReLU -> nn.MaxPool2d(2) on an
    NHWC map, the running statistics updated in place.  Saved for backward: z and the two [C] statistics - neither the normalised map
    nor the arg-max positions (the backward recomputes them from z).  dweight / dbias are ADDED into the parameters' .grad where that
    is the optimizer's bucket (then None goes back to autograd), as the convolutions' weight gradients are."""

    @staticmethod
    def forward(ctx, z, weight, bias, running_mean, running_var, num_batches_tracked, momentum, eps, sync=None):
        z = _req_map(z, "z")
        C = z.shape[3]
        weight, bias = _req(weight, "weight"), _req(bias, "bias")
        if tuple(weight.shape) != (C,) or tuple(bias.shape) != (C,):
            raise RuntimeError("bn_relu_maxpool2: weight and bias must be [C = %d]" % C)
        mean, invstd = _batch_stats(z, sync, eps, running_mean, running_var, num_batches_tracked, momentum)
        p = bn_pool_fwd(z, weight, bias, mean, invstd)
        ctx.save_for_backward(z, weight, bias, mean, invstd)
        ctx.sync = sync
        return p

    @staticmethod
    @once_differentiable
    def backward(ctx, dp):
        z, weight, bias, mean, invstd = ctx.saved_tensors
        dp = _req(dp, "dp")
        need = ctx.needs_input_grad
        sums = torch.empty((2, z.shape[3]), device=z.device, dtype=torch.float32)      # dgamma, dbeta of this rank's rows
        acc, (dw, db) = _channel_grads(need[1:3], (weight, bias), sums)
        bn_pool_bwd_sums(dp, z, weight, bias, mean, invstd, acc, sums)
        dz = None
        if need[0]:
            total = z.numel() // z.shape[3] * ctx.sync.world if _synced(ctx.sync) else None
            dz = bn_pool_bwd_dx(dp, z, weight, bias, mean, invstd, _total_sums(sums, ctx.sync), total)
        return dz, dw, db, None, None, None, None, None, None


def bn_relu_maxpool2(z, weight, bias, running_mean, running_var, num_batches_tracked, momentum=0.1, eps=1e-5, sync=None):
    """maxpool2(relu(batch_norm(z, batch statistics))) of an NHWC map -> [N, H/2, W/2, C]; differentiable in z, weight and bias
    (once); the running statistics and num_batches_tracked move as nn.BatchNorm2d's do in training mode.  sync (see DistSync): z is
    this rank's equal share of the batch, the statistics and dz are the whole batch's; None or world == 1: one process."""
    return BnReluMaxPool2Fn.apply(z, weight, bias, running_mean, running_var, num_batches_tracked, momentum, eps, sync)


class AbsDiffFn(Function):
    """|a - b| with torch's gradient: sign(a - b) * d for a, its negative for b, 0 where a == b.  halves: a and b are the two
    halves of ONE [2B, D] matrix (the pair batch encoded in one pass), whose gradient is written as one buffer."""

    @staticmethod
    def forward(ctx, a, b):
        ctx.halves = b is None
        if ctx.halves:
            e = _req(a, "e")
            if e.dim() != 2 or e.shape[0] % 2:
                raise RuntimeError("absdiff_halves: a [2B, D] matrix expected, got %s" % (tuple(e.shape),))
            B = e.shape[0] // 2
            y = _absdiff_fwd("absdiff_halves", e[:B], e[B:])[2]
            ctx.save_for_backward(e)
        else:
            a, b, y = _absdiff_fwd("absdiff_train", a, b)
            ctx.save_for_backward(a, b)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, d):
        lib = _lib.load()
        d = _req(d, "d")
        if ctx.halves:
            (e,) = ctx.saved_tensors
            a, b = e[:e.shape[0] // 2], e[e.shape[0] // 2:]
        else:
            a, b = ctx.saved_tensors
        if ctx.halves:
            g = torch.empty((2 * a.shape[0], a.shape[1]), device=a.device, dtype=torch.float32)
            da, db = g[:a.shape[0]], g[a.shape[0]:]
        else:
            da, db = torch.empty_like(a), torch.empty_like(a)
        check(lib.gim_absdiff_bwd(_p(a), _p(b), _p(d), _p(da), _p(db), a.numel(), _stream()), "absdiff_bwd")
        return (g, None) if ctx.halves else (da, db)


def absdiff_train(a, b):
    """|a - b|, elementwise and differentiable (ops.absdiff is the inference operator)."""
    return AbsDiffFn.apply(a, b)


def absdiff_halves(e):
    """|e[:B] - e[B:]| of a [2B, D] matrix, differentiable; the gradient w.r.t. e is produced as one buffer."""
    return AbsDiffFn.apply(e, None)


# --------------------------------------------------------------------------------------------
# training the ArcFace baseline (baseline_training.py): the passes of an IR-SE training step that are not convolutions, and the
# margin head (csrc/irse_train.hip).  fp32, one autograd.Function per pass, each once differentiable.  Gradients of per-channel
# parameters (gamma, beta, PReLU slope) are ADDED into the parameter's .grad where that is the optimizer's bucket (_grad_target),
# and None goes back to autograd - as BnReluMaxPool2Fn does.
# --------------------------------------------------------------------------------------------
def _req_chan(v, name, C):
    v = _req(v, name)
    if tuple(v.shape) != (C,):
        raise RuntimeError("%s must be [C = %d], got %s" % (name, C, tuple(v.shape)))
    return v


def _req_label(label, B):
    if not (torch.is_tensor(label) and label.is_cuda and label.dtype == torch.int64 and tuple(label.shape) == (B,)):
        raise RuntimeError("label must be a CUDA int64 tensor of shape [%d]" % B)
    return label if label.is_contiguous() else label.contiguous()


def bn_apply(z, weight, bias, mean, invstd, slope=None):
    """(z - mean) * invstd * weight + bias over the rows of z [..., C] with GIVEN statistics, then prelu(., slope); no autograd."""
    y = torch.empty_like(z)
    C = z.shape[-1]
    check(_lib.load().gim_bn_apply_fwd(_p(z), _p(weight), _p(bias), _p(mean), _p(invstd), _p(slope), _p(y), z.numel() // C, C, _stream()),
          "bn_apply_fwd")
    return y


def bn_bwd_sums(dy, z, weight, bias, mean, invstd, slope=None, acc=(None, None, None), out=None):
    """[3, C] = (dgamma, dbeta, dslope) of bn_apply over THIS tensor's rows (written to `out` where given; the dslope row only with a
    slope); acc: (weight.grad, bias.grad, slope.grad) buffers the sums are also ADDED to."""
    C = z.shape[-1]
    M = z.numel() // C
    sums = torch.empty((3, C), device=z.device, dtype=torch.float32) if out is None else out
    partials = _slab_partials(M, C, 3, z.device)
    check(_lib.load().gim_bn_bwd_reduce(_p(dy), _p(z), _p(weight), _p(bias), _p(mean), _p(invstd), _p(slope), _p(partials), _p(sums),
                                        _p(sums, C), _p(sums, 2 * C) if slope is not None else None, _p(acc[0]), _p(acc[1]), _p(acc[2]),
                                        M, C, _stream()), "bn_bwd_reduce")
    return sums


def bn_bwd_dx(dy, z, weight, bias, mean, invstd, slope, sums, total_rows=None):
    """dz of bn_apply from sums = (dgamma, dbeta).  total_rows: the rows of ALL ranks when sums are all ranks' totals (None: this
    tensor's own rows)."""
    lib = _lib.load()
    C = z.shape[-1]
    M = z.numel() // C
    dz = torch.empty_like(z)
    args = (_p(dy), _p(z), _p(weight), _p(bias), _p(mean), _p(invstd), _p(slope), _p(sums), _p(sums, C), _p(dz), M)
    if total_rows is None:
        check(lib.gim_bn_bwd_dx(*args, C, _stream()), "bn_bwd_dx")
    else:
        check(lib.gim_bn_bwd_dx_total(*args, int(total_rows), C, _stream()), "bn_bwd_dx_total")
    return dz


class BatchNormFn(Function):
    """y = batch_norm(z) with BATCH statistics over the rows of z [..., C] (nn.BatchNorm2d on an NHWC map, nn.BatchNorm1d on [B, C]
    in training mode), the running statistics updated in place; slope: the per-channel PReLU behind it, in the same pass.  Saved
    for backward: z and the two [C] statistics, not the normalised map."""

    @staticmethod
    def forward(ctx, z, weight, bias, slope, running_mean, running_var, num_batches_tracked, momentum, eps, sync=None):
        z, M, C = _req_rows(z, "z")
        weight, bias = _req_chan(weight, "weight", C), _req_chan(bias, "bias", C)
        slope = None if slope is None else _req_chan(slope, "slope", C)
        mean, invstd = _batch_stats(z, sync, eps, running_mean, running_var, num_batches_tracked, momentum)
        y = bn_apply(z, weight, bias, mean, invstd, slope)
        ctx.save_for_backward(z, weight, bias, mean, invstd, slope)
        ctx.sync = sync
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        z, weight, bias, mean, invstd, slope = ctx.saved_tensors
        C = z.shape[-1]
        dy = _req(dy, "dy")
        sums = torch.empty((3, C), device=z.device, dtype=torch.float32)      # dgamma, dbeta, dslope of this rank's rows
        need = ctx.needs_input_grad
        acc, (dw, db, ds) = _channel_grads(need[1:4], (weight, bias, slope), sums)
        bn_bwd_sums(dy, z, weight, bias, mean, invstd, slope, acc, sums)
        dz = None
        if need[0]:
            total = z.numel() // C * ctx.sync.world if _synced(ctx.sync) else None
            dz = bn_bwd_dx(dy, z, weight, bias, mean, invstd, slope, _total_sums(sums, ctx.sync), total)
        return dz, dw, db, ds, None, None, None, None, None, None


def batch_norm(z, weight, bias, running_mean, running_var, num_batches_tracked, momentum=0.1, eps=1e-5, slope=None, sync=None):
    """batch_norm(z, batch statistics) over the rows of z [..., C], optionally followed by prelu(., slope); differentiable in z, weight,
    bias and slope (once); the running statistics and num_batches_tracked move as nn.BatchNorm's do in training mode.  sync (see
    DistSync): z is this rank's equal share of the batch (one row is enough), the statistics and dz are the whole batch's; None or
    world == 1: one process."""
    return BatchNormFn.apply(z, weight, bias, slope, running_mean, running_var, num_batches_tracked, momentum, eps, sync)


class PReLUFn(Function):
    """y = x > 0 ? x : slope[c] * x over the last dim of x [..., C]; slope None: ReLU."""

    @staticmethod
    def forward(ctx, x, slope):
        lib = _lib.load()
        x, M, C = _req_rows(x, "x")
        slope = None if slope is None else _req_chan(slope, "slope", C)
        y = torch.empty_like(x)
        check(lib.gim_prelu_fwd(_p(x), _p(slope), _p(y), M, C, _stream()), "prelu_fwd")
        ctx.save_for_backward(x, slope)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        lib = _lib.load()
        x, slope = ctx.saved_tensors
        C = x.shape[-1]
        M = x.numel() // C
        dy = _req(dy, "dy")
        dx = torch.empty_like(x)
        sums = partials = None
        if slope is not None:
            sums = torch.empty((1, C), device=x.device, dtype=torch.float32)
            partials = _slab_partials(M, C, 1, x.device)
        (acc,), (ds,) = _channel_grads(ctx.needs_input_grad[1:2], (slope,), sums)
        check(lib.gim_prelu_bwd(_p(dy), _p(x), _p(slope), _p(dx), _p(partials), _p(sums), _p(acc), M, C, _stream()), "prelu_bwd")
        return dx, ds


def prelu(x, slope):
    """nn.PReLU(C) on the last dim (slope [C], any sign), or nn.ReLU when slope is None; differentiable (once)."""
    return PReLUFn.apply(x, slope)


def _strided_weight(w, Cin):
    """(storage view [Cout, KH, KH, Cin], logical) of a conv2d_strided weight.  logical: w is a convolution parameter as ops.conv2d
    takes it, [Cout, Cin, KH, KH] kept channels-last (weight_phys gives the view); else w is [Cout, KH, KH, Cin] itself, as
    conv2d_infer takes it.  Where both shapes fit (Cin == KH) the memory order decides: a channels-last parameter is not contiguous."""
    if w.dim() != 4:
        raise RuntimeError("conv2d_strided: weight %s is neither [Cout, KH, KH, Cin] nor a [Cout, Cin, KH, KH] parameter" % (tuple(w.shape),))
    Cout, a, b, c = w.shape
    as_storage, as_logical = (a == b and c == Cin), (b == c and a == Cin)
    if as_storage and as_logical:
        as_logical = not w.is_contiguous() and w.permute(0, 2, 3, 1).is_contiguous()
        as_storage = not as_logical
    if as_logical:
        return weight_phys(w), True
    if as_storage:
        return (w if w.is_contiguous() else w.contiguous()), False
    raise RuntimeError("conv2d_strided: weight %s does not match [Cout, KH, KH, Cin = %d] (or a [Cout, Cin = %d, KH, KH] parameter)"
                       % (tuple(w.shape), Cin, Cin))


def _note_strided(kind, cfg):
    N, Ho, Wo, Cin, Cout, KH, _ = cfg
    _FLOPS.setdefault((kind, cfg), [0, 2.0 * N * Ho * Wo * Cin * Cout * KH * KH])[0] += 1


class ConvStridedFn(Function):
    """y = conv(x, w, stride, padding = (KH - 1) / 2) + bias on an NHWC map, KH in {1, 3}: the library's strided training entries
    (gim_conv2d_strided_fwd / _dgrad / _wgrad).  A stride-2 convolution executes its own FLOPs in all three directions - it is not
    computed at full resolution and subsampled.  The weight and bias gradients go where ConvFn's go: ADDED into the parameter's
    existing .grad (FusedAdam's flat bucket; autograd then gets None and runs no AccumulateGrad kernel), returned otherwise; under
    ops.set_deterministic the forward and the dgrad never split K and the weight gradient's pixel slices are slabs added in a fixed
    order.  count_flops: ("strided_fwd" / "strided_dgrad" / "strided_wgrad", (N, Ho, Wo, Cin, Cout, KH, stride))."""

    @staticmethod
    def forward(ctx, x, w, bias, stride):
        lib = _lib.load()
        x = _req(x, "x")
        _req_w(w)
        if _PREC[0]:
            raise RuntimeError("conv2d_strided runs on the fp32 matrix path only (ops.set_matrix_path('fp32')): the strided launches "
                               "have no fp16 variant")
        if x.dim() != 4:
            raise RuntimeError("conv2d_strided: an NHWC map [N, H, W, Cin] expected, got %s" % (tuple(x.shape),))
        N, H, W, Cin = x.shape
        wp, logical = _strided_weight(w, Cin)
        Cout, KH = wp.shape[0], wp.shape[1]
        if bias is not None and tuple(_req(bias, "bias").shape) != (Cout,):
            raise RuntimeError("conv2d_strided: bias must be [Cout]")
        sh = _lib.GimInferConv(N, H, W, Cin, Cout, KH, stride)
        y = torch.empty((N, H // max(stride, 1), W // max(stride, 1), Cout), device=x.device, dtype=torch.float32)
        check(lib.gim_conv2d_strided_fwd(_p(x), _p(wp), _p(bias), _p(y), ctypes.byref(sh), _stream()), "conv2d_strided_fwd")
        ctx.save_for_backward(x, w, bias)
        ctx.cfg = (N, H, W, Cin, Cout, KH, stride, logical)
        if _FLOPS is not None:
            _note_strided("strided_fwd", (N, H // stride, W // stride, Cin, Cout, KH, stride))
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        lib = _lib.load()
        x, w, bias = ctx.saved_tensors
        N, H, W, Cin, Cout, KH, stride, logical = ctx.cfg
        dy = _req(dy, "dy")
        st, dev = _stream(), dy.device
        sh = _lib.GimInferConv(N, H, W, Cin, Cout, KH, stride)
        cfg = (N, H // stride, W // stride, Cin, Cout, KH, stride)
        det = 1 if _DETERMINISTIC[0] else 0
        need = ctx.needs_input_grad
        dx = dw = db = None
        if need[0]:
            wp = _strided_weight(w, Cin)[0]
            dx = torch.empty((N, H, W, Cin), device=dev, dtype=torch.float32)
            check(lib.gim_conv2d_strided_dgrad(_p(dy), _p(wp), _p(dx), ctypes.byref(sh), det, st), "conv2d_strided_dgrad")
            if _FLOPS is not None:
                _note_strided("strided_dgrad", cfg)
        want_b = bias is not None and need[2]
        if need[1]:
            # the parameter's .grad in the weight's own memory order (a [Cout, KH, KH, Cin] weight: the gradient tensor as it stands)
            if logical:
                acc_w = _grad_target(w)
            else:
                gw = w.grad
                acc_w = gw if (gw is not None and gw.is_cuda and gw.dtype == torch.float32 and gw.shape == w.shape and gw.is_contiguous()) else None
            acc_b = _grad_target(bias) if (want_b and acc_w is not None) else None
            if want_b and acc_b is None:
                acc_w = None      # one launch, one combine: both gradients are returned
            ws = None
            if det or _WGRAD_SLABS:
                nbytes = ctypes.c_int64(0)
                check(lib.gim_conv2d_strided_wgrad_workspace(ctypes.byref(sh), ctypes.byref(nbytes)), "conv2d_strided_wgrad_workspace")
                ws = torch.empty(max(nbytes.value // 4, 1), device=dev, dtype=torch.float32)
            if acc_w is not None:
                check(lib.gim_conv2d_strided_wgrad(_p(dy), _p(x), _p(acc_w), _p(acc_b), ctypes.byref(sh), 1, _p(ws), st), "conv2d_strided_wgrad")
            else:
                dwp = torch.empty((Cout, KH, KH, Cin), device=dev, dtype=torch.float32)
                if want_b:
                    db = torch.empty(Cout, device=dev, dtype=torch.float32)
                check(lib.gim_conv2d_strided_wgrad(_p(dy), _p(x), _p(dwp), _p(db), ctypes.byref(sh), 0, _p(ws), st), "conv2d_strided_wgrad")
                dw = dwp.permute(0, 3, 1, 2) if logical else dwp
            if _FLOPS is not None:
                _note_strided("strided_wgrad", cfg)
        elif want_b:
            db = torch.empty(Cout, device=dev, dtype=torch.float32)
            scratch = torch.empty(256 * Cout, device=dev, dtype=torch.float32)
            check(lib.gim_colsum(_p(dy), _p(db), _p(scratch), N * (H // stride) * (W // stride), Cout, st), "colsum")
        return dx, dw, db, None


def conv2d_strided(x, w, bias=None, stride=2):
    """y = conv(x, w, stride, padding = (KH - 1) / 2) + bias, differentiable in x, w and bias (ConvStridedFn).  x NHWC [N, H, W, Cin]
    (H, W powers of two >= 2); w [Cout, KH, KH, Cin] (the library's storage order) or a convolution parameter as ops.conv2d takes it
    ([Cout, Cin, KH, KH] kept channels-last - the form whose .grad lives in FusedAdam's bucket); KH in {1, 3}; stride in {1, 2}.
    Returns [N, H / stride, W / stride, Cout]."""
    return ConvStridedFn.apply(x, w, bias, stride)


class Subsample2Fn(Function):
    """y[n, i, j] = x[n, 2 i, 2 j] of an NHWC map with even H and W (MaxPool2d(1, 2); what a stride-2 convolution keeps of the
    stride-1 one).  The backward scatters into zeros in one pass."""

    @staticmethod
    def forward(ctx, x):
        lib = _lib.load()
        x = _req(x, "x")
        if x.dim() != 4 or x.shape[1] % 2 or x.shape[2] % 2 or x.shape[3] % 4:
            raise RuntimeError("subsample2: an NHWC map with even H, W and C %% 4 == 0 expected, got %s" % (tuple(x.shape),))
        N, H, W, C = x.shape
        y = torch.empty((N, H // 2, W // 2, C), device=x.device, dtype=torch.float32)
        check(lib.gim_subsample2_fwd(_p(x), _p(y), N, H, W, C, _stream()), "subsample2_fwd")
        ctx.cfg = (N, H, W, C)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        N, H, W, C = ctx.cfg
        dy = _req(dy, "dy")
        dx = torch.empty((N, H, W, C), device=dy.device, dtype=torch.float32)
        check(_lib.load().gim_subsample2_bwd(_p(dy), _p(dx), N, H, W, C, _stream()), "subsample2_bwd")
        return dx


def subsample2(x):
    return Subsample2Fn.apply(x)


class SETailFn(Function):
    """out = res * sigmoid(gate[n, c]) + shortcut[n, ::sstride, ::sstride, c] (the forward is the inference kernel gim_se_tail)."""

    @staticmethod
    def forward(ctx, res, gate, shortcut, sstride):
        if sstride not in (1, 2):      # the backward scatters the shortcut's gradient with subsample2_bwd
            raise RuntimeError("se_tail_train: sstride must be 1 or 2, got %s" % (sstride,))
        res, gate, out, _ = _se_tail_fwd("se_tail_train", res, gate, shortcut, sstride)
        ctx.save_for_backward(res, gate)
        ctx.sstride = sstride
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        lib = _lib.load()
        res, gate = ctx.saved_tensors
        N, Ho, Wo, C = res.shape
        dout = _req(dout, "dout")
        st = _stream()
        dres, dgate = torch.empty_like(res), torch.empty_like(gate)
        check(lib.gim_se_tail_bwd(_p(dout), _p(res), _p(gate), _p(dres), _p(dgate), N, Ho, Wo, C, st), "se_tail_bwd")
        dsc = None
        if ctx.needs_input_grad[2]:
            if ctx.sstride == 1:
                dsc = dout
            else:
                dsc = torch.empty((N, 2 * Ho, 2 * Wo, C), device=dout.device, dtype=torch.float32)
                check(lib.gim_subsample2_bwd(_p(dout), _p(dsc), N, 2 * Ho, 2 * Wo, C, st), "subsample2_bwd")
        return dres, dgate, dsc, None


def se_tail_train(res, gate, shortcut, sstride=1):
    """The end of an IR-SE unit, differentiable in res, gate and shortcut (ops.se_tail is the inference operator)."""
    return SETailFn.apply(res, gate, shortcut, sstride)


class DropoutFn(Function):
    """y = x * keep / (1 - p); keep is a hash of (seed, offset + element index): the backward recomputes it, no mask is stored."""

    @staticmethod
    def forward(ctx, x, p, seed, offset):
        x = _req(x, "x")
        if not 0.0 <= p < 1.0 or x.numel() % 4 or seed < 0 or offset < 0:
            raise RuntimeError("dropout: p in [0, 1), numel %% 4 == 0 and non-negative seed / offset expected")
        y = torch.empty_like(x)
        check(_lib.load().gim_dropout(_p(x), _p(y), x.numel(), p, seed, offset, _stream()), "dropout")
        ctx.cfg = (p, seed, offset)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        p, seed, offset = ctx.cfg
        dy = _req(dy, "dy")
        dx = torch.empty_like(dy)
        check(_lib.load().gim_dropout(_p(dy), _p(dx), dy.numel(), p, seed, offset, _stream()), "dropout")
        return dx, None, None, None


def dropout(x, p, seed, offset=0):
    """nn.Dropout(p) in training mode with the mask keyed by (seed, offset + element index); p == 0 copies x."""
    return DropoutFn.apply(x, float(p), int(seed), int(offset))


class L2NormRowsFn(Function):
    """x / |x| per row of [B, D]."""

    @staticmethod
    def forward(ctx, x):
        if x.dim() != 2 or x.shape[1] % 4:      # the backward kernel moves 16 bytes per access
            raise RuntimeError("l2norm_rows_train: [B, D] with D %% 4 == 0 expected, got %s" % (tuple(x.shape),))
        x, y = _l2norm_rows_fwd(x)
        ctx.save_for_backward(x)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dy = _req(dy, "dy")
        dx = torch.empty_like(x)
        check(_lib.load().gim_l2norm_rows_bwd(_p(dy), _p(x), _p(dx), x.shape[0], x.shape[1], _stream()), "l2norm_rows_bwd")
        return dx


def l2norm_rows_train(x):
    """x / |x| per row, differentiable (ops.l2norm_rows is the inference operator)."""
    return L2NormRowsFn.apply(x)


class ColL2NormFn(Function):
    """k / |k[:, j]| per COLUMN of k [E, N] (l2_norm(kernel, axis=0) of the ArcFace head)."""

    @staticmethod
    def forward(ctx, k):
        k = _req(k, "kernel")
        if k.dim() != 2:
            raise RuntimeError("col_l2norm: an [E, N] matrix expected, got %s" % (tuple(k.shape),))
        out = torch.empty_like(k)
        check(_lib.load().gim_col_l2norm_fwd(_p(k), _p(out), k.shape[0], k.shape[1], _stream()), "col_l2norm_fwd")
        ctx.save_for_backward(k)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dn):
        (k,) = ctx.saved_tensors
        dn = _req(dn, "dn")
        dk = torch.empty_like(k)
        check(_lib.load().gim_col_l2norm_bwd(_p(dn), _p(k), _p(dk), k.shape[0], k.shape[1], _stream()), "col_l2norm_bwd")
        return dk


def col_l2norm(k):
    return ColL2NormFn.apply(k)


def _margin_consts(s, m):
    return float(s), math.cos(m), math.sin(m), math.sin(m) * m, math.cos(math.pi - m)


class ArcMarginFn(Function):
    """ArcfaceHead.forward behind the cosine matrix: clamp to [-1, 1], the label column through the additive angular margin m
    (cos(theta + m), or cos - m sin m where theta + m would leave [0, pi]), everything times s."""

    @staticmethod
    def forward(ctx, cos, label, s, m):
        cos = _req(cos, "cos")
        if cos.dim() != 2:
            raise RuntimeError("arc_margin: a [B, classes] cosine matrix expected, got %s" % (tuple(cos.shape),))
        B, N = cos.shape
        label = _req_label(label, B)
        out = torch.empty_like(cos)
        check(_lib.load().gim_arcface_margin_fwd(_p(cos), label.data_ptr(), _p(out), B, N, *_margin_consts(s, m), _stream()), "arcface_margin_fwd")
        ctx.save_for_backward(cos, label)
        ctx.cfg = (s, m)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        cos, label = ctx.saved_tensors
        B, N = cos.shape
        dout = _req(dout, "dout")
        dcos = torch.empty_like(cos)
        check(_lib.load().gim_arcface_margin_bwd(_p(dout), _p(cos), label.data_ptr(), _p(dcos), B, N, *_margin_consts(*ctx.cfg), _stream()),
              "arcface_margin_bwd")
        return dcos, None, None, None


def arc_margin(cos, label, s=64.0, m=0.5):
    return ArcMarginFn.apply(cos, label, s, m)


class SoftmaxCEFn(Function):
    """(loss [B], correct [B]) of logits [B, classes] and int64 labels [B]: loss_b = logsumexp(row) - row[label], correct_b = 1.0
    where the row's first largest logit is the label's.  Only loss is differentiable."""

    @staticmethod
    def forward(ctx, logits, label):
        logits = _req(logits, "logits")
        if logits.dim() != 2:
            raise RuntimeError("softmax_ce: [B, classes] logits expected, got %s" % (tuple(logits.shape),))
        B, N = logits.shape
        label = _req_label(label, B)
        out = torch.empty((3, B), device=logits.device, dtype=torch.float32)      # loss, correct, lse
        check(_lib.load().gim_softmax_ce_fwd(_p(logits), label.data_ptr(), _p(out), _p(out, B), _p(out, 2 * B), B, N, _stream()), "softmax_ce_fwd")
        loss, correct = out[0], out[1]
        ctx.save_for_backward(logits, label, out[2])
        ctx.mark_non_differentiable(correct)
        return loss, correct

    @staticmethod
    @once_differentiable
    def backward(ctx, dloss, _dcorrect):
        logits, label, lse = ctx.saved_tensors
        B, N = logits.shape
        dloss = _req(dloss, "dloss")
        dlogits = torch.empty_like(logits)
        check(_lib.load().gim_softmax_ce_bwd(_p(dloss), _p(logits), label.data_ptr(), _p(lse), _p(dlogits), B, N, _stream()), "softmax_ce_bwd")
        return dlogits, None


def softmax_ce(logits, label):
    """-> (loss [B], correct [B])."""
    return SoftmaxCEFn.apply(logits, label)


# --------------------------------------------------------------------------------------------
# ROC statistics of two score sets as exact integer counts (authentication_eval.roc_statistics; csrc/roc.hip)
# --------------------------------------------------------------------------------------------
ROC_WORDS = 8       # GIM_ROC_WORDS of include/gim_hip.h


def roc_slices(n_cand, n_scores):
    """Number of slices a counts launch with `n_cand` candidates cuts `n_scores` = n_pos + n_neg scores into."""
    n = _lib.load().gim_roc_slices(n_cand, n_scores)
    if n <= 0:
        check(n, "roc_slices")
    return n


def _req_scores(t, name):
    t = _req(t, name)
    if t.dim() != 1 or t.numel() == 0:
        raise RuntimeError("%s must be a non-empty 1-D tensor, got %s" % (name, tuple(t.shape)))
    return t


def roc_counts(cand, pos, neg):
    """int64 [3, n_cand]: per candidate c the number of pos >= c, of neg < c and of neg == c (IEEE comparisons of fp32)."""
    cand, pos, neg = _req_scores(cand, "cand"), _req_scores(pos, "pos"), _req_scores(neg, "neg")
    counts = torch.empty((3, cand.numel()), device=cand.device, dtype=torch.int32)       # uint32 words; every count is below 2^31
    check(_lib.load().gim_roc_counts(_p(cand), cand.numel(), _p(pos), pos.numel(), _p(neg), neg.numel(), counts.data_ptr(), _stream()),
          "roc_counts")
    return counts.to(torch.int64)


def roc_record(pos, neg, counts=None):
    """(record, counts) of the candidates [pos; neg]: record = the ROC_WORDS int64 words of gim_roc_calibrate as a list of Python
    ints - the call's ONE host read - and counts the int32 [3, n_pos + n_neg] view of the workspace it filled.  `counts`: a CUDA
    int32 workspace of at least 3 * (n_pos + n_neg) words to use instead of a fresh one; the call zeroes what it uses."""
    pos, neg = _req_scores(pos, "pos"), _req_scores(neg, "neg")
    n = pos.numel() + neg.numel()
    if counts is None:
        counts = torch.empty(3 * n, device=pos.device, dtype=torch.int32)
    elif not (counts.is_cuda and counts.dtype == torch.int32 and counts.is_contiguous() and counts.numel() >= 3 * n):
        raise RuntimeError("roc_record: counts must be a contiguous CUDA int32 workspace of at least %d words" % (3 * n))
    record = torch.empty(ROC_WORDS, device=pos.device, dtype=torch.int64)
    check(_lib.load().gim_roc_calibrate(_p(pos), pos.numel(), _p(neg), neg.numel(), counts.data_ptr(), record.data_ptr(), _stream()),
          "roc_calibrate")
    return record.tolist(), counts.view(-1)[:3 * n].view(3, n)
