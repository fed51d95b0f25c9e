"""Fused multi-tensor Adam on flat buffers + the data-parallel gradient exchange.

Replaces the two ``torch.optim.Adam`` instances of the reference trainer
(training/gim_img_trainer.py:50-58) and the gradient reduce-add of ``nn.DataParallel``
(training/gim_img_training.py:409):

  * all parameters of an optimizer live in ONE flat fp32 buffer (parameters become views into it; conv
    weights keep their channels-last storage), gradients in a second flat buffer, Adam moments in two more;
  * ``step()`` = [one RCCL all-reduce of the flat gradient buffer when torch.distributed is initialised]
    + ONE kernel launch (gim_adam_step) with per-parameter-group learning rates read from device memory;
  * ``zero_grad()`` = one memset of the flat gradient buffer.

``state_dict()`` / ``load_state_dict()`` keep torch.optim.Adam's format (per-parameter ``step`` /
``exp_avg`` / ``exp_avg_sq``; group keys lr, betas, eps, weight_decay, amsgrad), so reference checkpoints load.
"""
import math
import os
from contextlib import contextmanager

import torch
import torch.distributed as dist

from . import _lib
from ._lib import check


def _phys(t):
    """Memory-order view of a parameter-like tensor (conv weights are stored channels-last)."""
    if t.dim() == 4:
        return t.permute(0, 2, 3, 1)
    return t


def _view_like(flat_slice, ref):
    """View of a flat slice with the logical shape of ``ref`` (channels-last strides for 4-D)."""
    if ref.dim() == 4:
        co, ci, kh, kw = ref.shape
        return flat_slice.view(co, kh, kw, ci).permute(0, 3, 1, 2)
    return flat_slice.view(ref.shape)


def weights_epoch(p):
    """Number of FusedAdam updates applied to parameter ``p``.  The Adam kernel writes parameters through raw
    pointers, which torch's version counters do not see; caches derived from a weight (folded conv weights) key on
    (p._version, weights_epoch(p))."""
    return getattr(p, "_gim_epoch", 0)


def _pad(n, align=64):
    return (n + align - 1) // align * align


# rehearsal switch: issue the collective even with one rank (exercises the RCCL call path on a one-GPU box)
_FORCE_ALLREDUCE = os.environ.get("GIM_FORCE_ALLREDUCE") is not None


def all_reduce_grads_(flat_g, timing=None):
    """Data-parallel gradient exchange: ONE all-reduce(sum) of a flat gradient bucket over RCCL/xGMI (gloo in
    the CPU tests).  Each rank's bucket holds the gradient of its local mean loss, so the global-batch
    gradient is the returned scale (1/world_size) times the reduced bucket; the scale is folded into the
    Adam kernel.  No-op (scale 1) when torch.distributed is not initialised.
    timing: a list that receives (event before, event after) on the caller's stream per collective (bench.py: `allreduce_ms`;
    the events bracket the collective as the STEP sees it - RCCL runs it on its own stream and the caller's stream waits for it)."""
    if dist.is_available() and dist.is_initialized() and (dist.get_world_size() > 1 or _FORCE_ALLREDUCE):
        if timing is not None and flat_g.is_cuda:
            cur = torch.cuda.current_stream()
            e0 = cur.record_event(torch.cuda.Event(enable_timing=True))
            dist.all_reduce(flat_g, op=dist.ReduceOp.SUM)
            timing.append((e0, cur.record_event(torch.cuda.Event(enable_timing=True))))
        else:
            dist.all_reduce(flat_g, op=dist.ReduceOp.SUM)
        return 1.0 / dist.get_world_size()
    return 1.0


class LossScaler:
    """Dynamic loss scale of the fp16 matrix path, resident on the device (layout: include/gim_hip.h, gim_adam_step_scaled).
    The step functions differentiate scale_loss(loss); FusedAdam.step (loss_scaler set) tests the gradient bucket, skips the
    update on inf / NaN and halves the scale, and doubles it after growth_interval clean steps in a row.  Nothing here reads
    the device except state() (and state_dict(), which calls it)."""
    WORDS = 8

    def __init__(self, device, init=4096.0, growth_interval=2000, min_scale=1.0):
        self.device = torch.device(device)
        self.words = torch.zeros(self.WORDS, dtype=torch.int32, device=self.device)
        self._set(float(init), int(growth_interval), 0, 0, float(min_scale), 0)

    def _set(self, scale, interval, clean, skipped, min_scale, last_overflow):
        if not (scale > 0 and min_scale > 0 and interval >= 1):
            raise ValueError("LossScaler: scale and min_scale must be positive, growth_interval >= 1")
        host = torch.zeros(self.WORDS, dtype=torch.int32)
        host[:2].view(torch.float32).copy_(torch.tensor([scale, 1.0 / scale]))
        host[6:7].view(torch.float32).fill_(min_scale)
        host[2], host[3], host[5], host[7] = interval, clean, skipped, last_overflow
        self.words.copy_(host)
        self._scale = self.words[0:1].view(torch.float32)   # the device scalar scale_loss multiplies by

    def scale_loss(self, loss):
        """loss * scale as an engine op on the device scalar (no host read, graph-capture safe)."""
        from . import ops
        return ops.MulScalarFn.apply(loss.reshape(1), self._scale).reshape(loss.shape)

    def state(self):
        """{"scale", "clean_steps", "skipped", "last_overflow", "growth_interval", "min_scale"} - synchronises."""
        w = self.words.cpu()
        f = w.view(torch.float32)
        return {"scale": float(f[0]), "clean_steps": int(w[3]), "skipped": int(w[5]), "last_overflow": bool(w[7]),
                "growth_interval": int(w[2]), "min_scale": float(f[6])}

    def state_dict(self):
        return self.state()

    def load_state_dict(self, sd):
        cur = self.state()
        cur.update(sd)
        self._set(float(cur["scale"]), int(cur["growth_interval"]), int(cur["clean_steps"]), int(cur["skipped"]),
                  float(cur["min_scale"]), int(bool(cur["last_overflow"])))


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=0, amsgrad=False)
        super().__init__(params, defaults)
        self._built = False
        self._host_step = 0
        self._lr_cache = None
        self.grad_divisor = None  # set by dp: world size for the post-all-reduce average
        self.loss_scaler = None        # a LossScaler: step() tests the bucket, skips on inf / NaN and un-scales by the DEVICE scale
        self.allreduce_timing = None   # a list: step() appends the (before, after) events of its gradient all-reduce (bench.py)
        self._avg_decay = None         # averaged agent (enable_averaging): the decay; flat_avg exists from the build on
        self.flat_avg = None
        self._avg_carry = None         # {parameter: average} waiting for the next (re)build of the flat buffers
        self._swapped = False          # inside averaged_weights(): flat_p holds the averages
        self._omega = None             # optimistic step (enable_optimism): omega; flat_prev exists from the build on
        self.flat_prev = None
        self._prev_carry = None        # {parameter: previous direction} waiting for the next (re)build of the flat buffers

    def dynamic_scaler(self):
        """The LossScaler the step functions use (created on first use from ops.set_loss_scale's settings), or None when the loss
        scale is static or the matrix path fp32."""
        from . import ops
        if ops.matrix_path() != "fp16" or ops.loss_scale_mode() != "dynamic":
            return None
        if self.loss_scaler is None:
            self.loss_scaler = LossScaler(self._all_params()[0].device, **ops.dynamic_loss_scale_defaults())
        return self.loss_scaler

    # ------------------------------------------------------------------ flat storage
    def _all_params(self):
        return [p for g in self.param_groups for p in g["params"]]

    def _build(self):
        params = self._all_params()
        dev = params[0].device
        if dev.type != "cuda":
            raise RuntimeError("FusedAdam runs on the GPU only (parameters are on %s); there is no CPU fallback" % dev)
        # every tensor starts on a 256-byte boundary of the flat buffers: the conv kernels need 16-byte
        # aligned weights for their vector loads (the padding elements are zeros and stay zeros)
        total = sum(_pad(p.numel()) for p in params)
        self.flat_p = torch.zeros(total, device=dev, dtype=torch.float32)
        self.flat_g = torch.zeros(total, device=dev, dtype=torch.float32)
        self.flat_m = torch.zeros(total, device=dev, dtype=torch.float32)
        self.flat_v = torch.zeros(total, device=dev, dtype=torch.float32)
        self._offsets = {}
        seg_end = []
        o = 0
        with torch.no_grad():
            for g in self.param_groups:
                for p in g["params"]:
                    n = p.numel()
                    self.flat_p[o:o + n].copy_(_phys(p.data).reshape(-1))
                    old_grad = p.grad
                    p.data = _view_like(self.flat_p[o:o + n], p)
                    gv = _view_like(self.flat_g[o:o + n], p)
                    if old_grad is not None:
                        gv.copy_(old_grad)
                    p.grad = gv
                    st = self.state.get(p)
                    if st:  # state imported by load_state_dict before the buffers existed
                        _view_like(self.flat_m[o:o + n], p).copy_(st["exp_avg"])
                        _view_like(self.flat_v[o:o + n], p).copy_(st["exp_avg_sq"])
                        self._host_step = max(self._host_step, int(st["step"]))
                    self._offsets[p] = (o, n)
                    o += _pad(n)
                seg_end.append(o)
        self._seg_end = torch.tensor(seg_end, dtype=torch.int64, device=dev)
        self._lr_dev = torch.zeros(len(seg_end), dtype=torch.float32, device=dev)
        self._lr_cache = None   # a rebuild after the first step: the new table is zeros until _push_lrs fills it
        self._step_dev = torch.full((1,), self._host_step, dtype=torch.int32, device=dev)
        self._built = True
        self._publish_state()
        if self._avg_decay is not None:
            self._alloc_average()
        if self._omega is not None:
            self._alloc_prev()

    def _publish_state(self):
        """Expose the flat moments through ``self.state`` in torch.optim.Adam's per-parameter format."""
        for p, (o, n) in self._offsets.items():
            self.state[p] = {
                "step": torch.tensor(float(self._host_step)),
                "exp_avg": _view_like(self.flat_m[o:o + n], p),
                "exp_avg_sq": _view_like(self.flat_v[o:o + n], p),
            }

    def _ensure(self):
        if not self._built:
            self._build()
            return
        for p, (o, n) in self._offsets.items():
            if p.data_ptr() != self.flat_p.data_ptr() + 4 * o:  # e.g. module.to() / load after build
                self._sync_host_step()
                if self.flat_avg is not None:   # the averages move with their parameters, as the moments do through self.state
                    self._avg_carry = self._average_views()
                if self.flat_prev is not None:  # and so do the previous directions: a rebuild never zeroes them
                    self._prev_carry = self._prev_views()
                self._built = False
                self._build()
                return

    def _sync_host_step(self):
        """With a loss scaler only the device counter knows how many steps were applied (a skipped one does not count)."""
        if self.loss_scaler is not None:
            self._host_step = int(self._step_dev.item())

    def _sync_grads(self):
        """Gradients normally accumulate in place into the flat buffer; re-home any that did not."""
        base = self.flat_g.data_ptr()
        for p, (o, n) in self._offsets.items():
            g = p.grad
            if g is None:
                p.grad = _view_like(self.flat_g[o:o + n], p)
            elif g.data_ptr() != base + 4 * o:
                gv = _view_like(self.flat_g[o:o + n], p)
                gv.copy_(g)
                p.grad = gv

    # ------------------------------------------------------------------ optimizer protocol
    def zero_grad(self, set_to_none=False):
        self._not_swapped("zero_grad()")
        self._ensure()
        from . import ops
        ops.reset_wgrad_queues()
        self.flat_g.zero_()
        self._sync_grads()

    def flat_grad(self):
        self._ensure()
        self._sync_grads()
        return self.flat_g

    def _push_lrs(self):
        lrs = [float(g["lr"]) for g in self.param_groups]
        if lrs != self._lr_cache:
            self._lr_dev.copy_(torch.tensor(lrs, dtype=torch.float32), non_blocking=False)
            self._lr_cache = lrs

    @torch.no_grad()
    def step(self, closure=None, grad_scale=1.0, micro_batches=1):
        """grad_scale multiplies the gradient bucket inside the Adam kernel (together with the 1 / world_size of the data-parallel
        average): 1 / S after a backward pass of S * loss (the loss scale of the fp16 matrix path, ops.loss_scale).  With a
        loss_scaler the kernel takes 1 / S from the scaler's device state (pass grad_scale = 1) and the update is skipped when the
        bucket - after the all-reduce, so on every rank alike - holds an inf or a NaN.
        micro_batches = A: the bucket holds the SUM of the gradients of A local mean losses (an accumulated step of
        gim_img_training: A backward passes since zero_grad()); the kernel's scale takes the 1 / A of their mean as it takes the
        1 / world_size, so N ranks x A micro-batches are scaled by 1 / (N A) and all-reduced once."""
        assert closure is None
        self._not_swapped("step()")
        if micro_batches != 1:
            grad_scale = grad_scale / micro_batches
        lib = _lib.load()
        self._ensure()
        self._sync_grads()
        self._push_lrs()
        scale = all_reduce_grads_(self.flat_g, self.allreduce_timing)
        g0 = self.param_groups[0]
        for g in self.param_groups:
            assert g["betas"] == g0["betas"] and g["eps"] == g0["eps"], "one (betas, eps) per optimizer"
        args = (self.flat_p.data_ptr(), self.flat_g.data_ptr(), self.flat_m.data_ptr(), self.flat_v.data_ptr(),
                self.flat_p.numel(), self._seg_end.data_ptr(), self._lr_dev.data_ptr(), len(self.param_groups),
                g0["betas"][0], g0["betas"][1], g0["eps"], scale * grad_scale, self._step_dev.data_ptr())
        if self.loss_scaler is not None:
            check(lib.gim_adam_step_scaled(*args, self.loss_scaler.words.data_ptr(), torch.cuda.current_stream().cuda_stream), "adam_step_scaled")
        else:
            check(lib.gim_adam_step(*args, torch.cuda.current_stream().cuda_stream), "adam_step")
        if self._omega is not None:
            # one correction per step(), behind the Adam launches and in front of the average, which must see the corrected weights
            self._launch_optimism(self._omega)
        if self._avg_decay is not None:
            # one update per step(), behind the Adam launches on the same stream; with a loss scaler the kernel reads the scaler's
            # "last call skipped" word (scaler_update_kernel has just written it): a skipped step leaves the average alone
            check(lib.gim_ema_update(self.flat_avg.data_ptr(), self.flat_p.data_ptr(), self.flat_p.numel(), self._avg_decay,
                                     self.loss_scaler.words.data_ptr() if self.loss_scaler is not None else None,
                                     torch.cuda.current_stream().cuda_stream), "ema_update")
        self.note_steps(1)

    def note_steps(self, k):
        """Host-side bookkeeping of k applied updates (called by step(); call it yourself after replaying a captured
        hipGraph that contains step(), since the replay does not run this Python code)."""
        self._host_step += k
        for p in self._offsets:
            p._gim_epoch = getattr(p, "_gim_epoch", 0) + k

    def _bump_epochs(self):
        """Every cached copy of every parameter goes stale (ops._WT_CACHE keys on weights_epoch); Adam's step count stays."""
        for p in self._offsets:
            p._gim_epoch = getattr(p, "_gim_epoch", 0) + 1

    # ------------------------------------------------------------------ averaged agent
    # flat_avg = decay * flat_avg + (1 - decay) * flat_p after every applied step (training/utils.py:96-101, accumulate), in the
    # layout of flat_p (padding zeros, which both kernels keep).  It starts as a copy of the weights, so there is no bias to correct.
    @property
    def averaging(self):
        """The decay of the weight average, or None when averaging is off."""
        return self._avg_decay

    def enable_averaging(self, decay):
        d = float(decay)
        d32 = torch.tensor(d, dtype=torch.float32).item() if not math.isnan(d) else d   # what the kernel is given
        if not (0.0 <= d32 < 1.0):
            raise ValueError("enable_averaging: decay must be in [0, 1) as a float32, got %r" % (decay,))
        self._avg_decay = d
        if self._built and self.flat_avg is None:
            self._alloc_average()

    def disable_averaging(self):
        self._not_swapped("disable_averaging()")
        self._avg_decay = self.flat_avg = self._avg_carry = None

    def _alloc_average(self):
        carry, self._avg_carry = self._avg_carry or {}, None
        self.flat_avg = self.flat_p.clone()
        with torch.no_grad():
            for p, (o, n) in self._offsets.items():
                if p in carry:
                    _view_like(self.flat_avg[o:o + n], p).copy_(carry[p])

    def _average_views(self):
        return {p: _view_like(self.flat_avg[o:o + n], p) for p, (o, n) in self._offsets.items()}

    def _averaging_ready(self, what):
        if self._avg_decay is None:
            raise RuntimeError("FusedAdam.%s: averaging is off (enable_averaging)" % what)
        self._not_swapped(what)
        self._ensure()

    def _not_swapped(self, what):
        if self._swapped:
            raise RuntimeError("FusedAdam.%s inside averaged_weights(): the parameters hold the averages" % what)

    def average_state(self):
        """{parameter: its average}, views of the flat buffer in each parameter's logical shape."""
        self._averaging_ready("average_state()")
        return self._average_views()

    @torch.no_grad()
    def load_average(self, mapping):
        """Copy averages in: {parameter: tensor of its shape}; parameters the mapping does not have keep theirs."""
        self._averaging_ready("load_average()")
        views = self._average_views()
        for p, t in mapping.items():
            views[p].copy_(t)

    @torch.no_grad()
    def reset_average(self):
        """average = weights, as at enable_averaging."""
        self._averaging_ready("reset_average()")
        self.flat_avg.copy_(self.flat_p)

    def _exchange(self):
        check(_lib.load().gim_buffer_exchange(self.flat_p.data_ptr(), self.flat_avg.data_ptr(), self.flat_p.numel(),
                                              torch.cuda.current_stream().cuda_stream), "buffer_exchange")
        self._bump_epochs()

    @contextmanager
    def averaged_weights(self):
        """Inside, every parameter holds its average: flat_p and flat_avg trade contents (one kernel, no pointer moves, so
        _ensure() sees nothing) and every cached weight copy goes stale; the exit trades them back, also when the body raises.
        step() and zero_grad() raise inside, and so does a second averaged_weights()."""
        from . import ops
        self._averaging_ready("averaged_weights()")
        ops.join_lanes()   # a discriminator step still running on lane 1 (gim_step(defer_join=True)) writes these weights
        self._exchange()
        self._swapped = True
        try:
            yield self
        finally:
            self._exchange()
            self._swapped = False

    # ------------------------------------------------------------------ optimistic step
    # Optimistic Adam (Daskalakis et al., "Training GANs with Optimism", Algorithm 1): the step along d_t + omega (d_t - d_{t-1}), d_t =
    # Adam's bias-corrected direction.  flat_prev holds d_{t-1} in the layout of flat_p; it starts as zeros, so with omega = 1 the
    # first step is 2 lr d_1, as in the paper.  One streaming kernel behind Adam (csrc/oadam.hip), which also keeps d_t.
    @property
    def optimism(self):
        """omega of the optimistic step, or None when it is off."""
        return self._omega

    def enable_optimism(self, omega):
        self._not_swapped("enable_optimism()")
        w = float(omega)
        w32 = torch.tensor(w, dtype=torch.float32).item() if not math.isnan(w) else w   # what the kernel is given
        if not (0.0 < w32 <= 1.0):
            raise ValueError("enable_optimism: omega must be in (0, 1] as a float32, got %r" % (omega,))
        self._omega = w
        if self._built and self.flat_prev is None:
            self._alloc_prev()

    def disable_optimism(self):
        self._not_swapped("disable_optimism()")
        self._omega = self.flat_prev = self._prev_carry = None

    def _alloc_prev(self):
        carry, self._prev_carry = self._prev_carry or {}, None
        self.flat_prev = torch.zeros_like(self.flat_p)
        with torch.no_grad():
            for p, (o, n) in self._offsets.items():
                if p in carry:
                    _view_like(self.flat_prev[o:o + n], p).copy_(carry[p])

    def _prev_views(self):
        return {p: _view_like(self.flat_prev[o:o + n], p) for p, (o, n) in self._offsets.items()}

    def _optimism_ready(self, what):
        if self._omega is None:
            raise RuntimeError("FusedAdam.%s: the optimistic step is off (enable_optimism)" % what)
        self._not_swapped(what)
        self._ensure()

    def _launch_optimism(self, omega, guarded=True):
        """gim_adam_optimism on the current stream; omega = 0 only records the direction.  The kernel reads the step counter and the
        learning rates on the device and, when guarded behind a loss scaler, the scaler's "last call skipped" word."""
        g0 = self.param_groups[0]
        scaler = self.loss_scaler if guarded else None
        check(_lib.load().gim_adam_optimism(
            self.flat_p.data_ptr(), self.flat_prev.data_ptr(), self.flat_m.data_ptr(), self.flat_v.data_ptr(), self.flat_p.numel(),
            self._seg_end.data_ptr(), self._lr_dev.data_ptr(), len(self.param_groups), g0["betas"][0], g0["betas"][1], g0["eps"],
            omega, self._step_dev.data_ptr(), scaler.words.data_ptr() if scaler is not None else None,
            torch.cuda.current_stream().cuda_stream), "adam_optimism")

    def optimism_state(self):
        """{parameter: the direction d of its last applied step}, views of the flat buffer in each parameter's logical shape."""
        self._optimism_ready("optimism_state()")
        return self._prev_views()

    @torch.no_grad()
    def load_optimism(self, mapping):
        """Copy previous directions in: {parameter: tensor of its shape}; parameters the mapping does not have keep theirs."""
        self._optimism_ready("load_optimism()")
        views = self._prev_views()
        for p, t in mapping.items():
            views[p].copy_(t)

    @torch.no_grad()
    def prime_optimism(self):
        """prev = Adam's direction from the current moments and step count, the parameters untouched: after loading an Adam state
        that came without directions, the next step is then a plain Adam step up to the change of direction, not a doubled one.
        Nothing to record while no step has been applied."""
        self._optimism_ready("prime_optimism()")
        self._sync_host_step()
        if self._host_step == 0:
            return
        self._launch_optimism(0.0, guarded=False)   # whatever became of the last step before the state was saved

    # ------------------------------------------------------------------ checkpoint format
    def state_dict(self):
        if self._built:
            self._sync_host_step()   # "step" from the device counter: _host_step would count a skipped step
            self._publish_state()
        return super().state_dict()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        steps = [int(s["step"]) for s in self.state.values() if "step" in s]
        self._host_step = max(steps) if steps else 0
        if self._built:
            with torch.no_grad():
                for p, (o, n) in self._offsets.items():
                    st = self.state.get(p)
                    if st and "exp_avg" in st:
                        _view_like(self.flat_m[o:o + n], p).copy_(st["exp_avg"])
                        _view_like(self.flat_v[o:o + n], p).copy_(st["exp_avg_sq"])
                self._step_dev.fill_(self._host_step)
            self._publish_state()
        self._lr_cache = None
