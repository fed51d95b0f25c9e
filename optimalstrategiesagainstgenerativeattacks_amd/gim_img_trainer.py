"""GIMImgTrainer on the MI355X engine: host-side mirror of the reference's ``training/gim_img_trainer.py``
(constructor, the three ``forward`` modes and their return tuples, optimizer / scheduler attributes,
checkpoint hooks, lr / global-step accessors).

Differences that do not change any result of the training loop:
  * both optimizers are ``FusedAdam`` (one flat-buffer kernel per step, RCCL all-reduce built in);
  * in ``impersonator_forward`` the authenticator's parameters are frozen for the duration of the forward, so
    the generator step does not compute the discriminator weight gradients that the reference computes and
    then discards (``authenticator_opt.zero_grad()`` at training/gim_img_training.py:172) - SURVEY.md 8(a);
  * the R1 term (``reg_param > 0``) differentiates the authenticator's input gradient through the same HIP kernels
    (ops.ConvDgradFn and friends); no torch operator is on that path either.
"""
import os
from contextlib import ExitStack, contextmanager

import torch
import torch.nn as nn
import torch.optim as optim

from . import ops
from .optim import FusedAdam
from .training_utils import CheckpointIO, GlobalStep, compute_grad2, num_parameters


@contextmanager
def _frozen(module):
    ps = [p for p in module.parameters() if p.requires_grad]
    for p in ps:
        p.requires_grad_(False)
    try:
        yield
    finally:
        for p in ps:
            p.requires_grad_(True)


class GimTrainerBase(nn.Module):
    """What the image and the Gaussian trainer share: the mode-string forward, the BCE game losses, the assembly of the
    discriminator step's 9-tuple, checkpoint wiring and the global-step counter (training/gim_img_trainer.py:79-94,158-172,
    training/gim_gaussian_trainer.py - the reference writes these twice)."""
    CHECKPOINT_DIR = "ckpts"
    MODES = ("authenticator_forward", "impersonator_forward", "impersonator_sample")
    CHECKPOINT_KEYS = ("authenticator", "impersonator", "authenticator_opt", "impersonator_opt")

    def _init_agents(self, m, n, k, authenticator, impersonator, reg_param, remove_noise_mean):
        self.m, self.n, self.k = m, n, k
        self.authenticator, self.impersonator = authenticator, impersonator
        self.reg_param, self.remove_noise_mean = reg_param, remove_noise_mean
        self._global_step = GlobalStep()

    def _init_checkpoints(self, outdir):
        for label, net in (("Authenticator", self.authenticator), ("impersonator", self.impersonator)):
            print("{} has {} parameters".format(label, num_parameters(net.parameters())))
        self.checkpoint_dir = os.path.join(outdir, self.CHECKPOINT_DIR)
        self.checkpoint_io = CheckpointIO(checkpoint_dir=self.checkpoint_dir)
        self.checkpoint_io.register_modules(**{key: getattr(self, key) for key in self.CHECKPOINT_KEYS},   # the dict keys of the .pt file
                                            global_step=self._global_step)

    def forward(self, mode, **kwargs):
        """One entry point with a mode string, so that a data-parallel wrapper sees a plain nn.Module.forward."""
        if mode not in self.MODES:
            raise ValueError("unsupported mode")
        return getattr(self, mode)(**kwargs)

    def gan_loss(self, dis_out, target, reduce=False):
        """BCE-with-logits against a constant target, per episode (training/gim_img_trainer.py:90-94)."""
        loss = ops.bce_logits(dis_out, float(target))
        return (loss.mean() if reduce else loss).squeeze()

    def _discriminator_terms(self, out_on_real, out_on_fake_fn, real_sample, si_sample, fake_sample, grad):
        """The 9-tuple of authenticator_forward from the logits on the real sample and a callable for the logits on the fake one
        (called AFTER the R1 term, as the reference orders its two discriminator calls: training/gim_img_trainer.py:102-123)."""
        loss_on_real = self.gan_loss(dis_out=out_on_real, target=1.)
        if grad and self.reg_param > 0:
            reg = self.reg_param * compute_grad2(out_on_real, (real_sample, si_sample))
        else:
            reg = torch.zeros_like(loss_on_real)
        out_on_fake = out_on_fake_fn()
        loss_on_fake = self.gan_loss(dis_out=out_on_fake, target=0.)
        with torch.no_grad():
            pred_on_real, pred_on_fake = out_on_real.detach() >= 0, out_on_fake.detach() >= 0
        return (loss_on_real + loss_on_fake + reg, loss_on_real.detach(), loss_on_fake.detach(), reg, out_on_real.detach(),
                out_on_fake.detach(), pred_on_real, pred_on_fake, fake_sample.detach())

    def _wants_input_grad(self, real_sample, si_sample):
        if self.reg_param > 0:   # R1 differentiates the logits w.r.t. the discriminator's inputs (training/gim_img_trainer.py:98-100)
            real_sample.requires_grad_()
            si_sample.requires_grad_()

    def impersonator_sample(self, leaked_sample, z=None):
        with torch.no_grad():
            return self.impersonator(leaked_sample=leaked_sample, n=self.n, remove_noise_mean=self.remove_noise_mean, z=z)

    # ---- averaged agents: an exponential moving average of each agent's weights, kept by its optimizer (optim.FusedAdam) ----
    def _agents(self):
        return (("impersonator", self.impersonator, self.impersonator_opt), ("authenticator", self.authenticator, self.authenticator_opt))

    def _init_averaging(self, im_ema_decay, au_ema_decay):
        """None = off: no buffer, no launch, no checkpoint entry.  Call after _init_checkpoints."""
        for (_, _, opt), decay in zip(self._agents(), (im_ema_decay, au_ema_decay)):
            if decay is not None:
                opt.enable_averaging(decay)
        self._averaged = _Averaged(self)
        self.checkpoint_io.register_optional(averaged=self._averaged)

    def averages(self):
        """True when at least one agent keeps an average."""
        return any(opt.averaging is not None for _, _, opt in self._agents())

    @contextmanager
    def averaged(self):
        """Inside, every agent that averages runs on its averaged weights, and both agents are in eval mode: a train-mode forward
        runs a power iteration and would move the live weight_u / weight_v from the averaged weights.  sigma is u^T W_avg v with
        the live u, v.  The previous modes come back on exit, and the live weights bit for bit."""
        agents = self._agents()
        modes = [net.training for _, net, _ in agents]
        with ExitStack() as stack:
            for _, _, opt in agents:
                if opt.averaging is not None:
                    stack.enter_context(opt.averaged_weights())
            try:
                for _, net, _ in agents:
                    net.eval()
                yield self
            finally:
                for (_, net, _), mode in zip(agents, modes):
                    net.train(mode)

    # ---- optimistic updates: each optimizer steps along d_t + omega (d_t - d_{t-1}) (optim.FusedAdam.enable_optimism) ----
    def _init_optimism(self, im_optimism, au_optimism):
        """None = off: no buffer, no launch, no checkpoint entry.  Call after _init_checkpoints."""
        for (_, _, opt), omega in zip(self._agents(), (im_optimism, au_optimism)):
            if omega is not None:
                opt.enable_optimism(omega)
        self._optimism = _Optimism(self)
        self.checkpoint_io.register_optional(optimism=self._optimism)

    def resume_from_ckpt(self, ckpt_path):
        averaged, optimism = getattr(self, "_averaged", None), getattr(self, "_optimism", None)
        if averaged is not None:
            averaged.loaded = set()
        if optimism is not None:
            optimism.loaded = set()
        found = self.checkpoint_io.load(ckpt_path) != (-1, -1)
        if optimism is not None and found:
            # a file without the entry (or without this agent): the previous direction is the one of the loaded Adam state, so the
            # first step after resuming is a plain Adam step, not a doubled one
            for name, _, opt in self._agents():
                if opt.optimism is not None and name not in optimism.loaded:
                    opt.prime_optimism()
        if averaged is not None and found:
            # a file without the entry (or without this agent): the average starts from the loaded weights
            for name, _, opt in self._agents():
                if opt.averaging is not None and name not in averaged.loaded:
                    opt.reset_average()
        print("Resuming training from iteration {}".format(self.global_step))

    def get_global_step(self):
        return self._global_step.get()

    def do_global_step(self):
        return self._global_step.step()

    @property
    def global_step(self):
        return self.get_global_step()


class _LossScalers:
    """Checkpoint entry "loss_scalers": the dynamic loss scale of each optimizer (fp16 matrix path, GIM_FP16_LOSS_SCALE=dynamic).
    Absent in every other mode, so the file then has the reference's keys only."""

    def __init__(self, **opts):
        self.opts = opts

    def state_dict(self):
        scalers = {name: opt.dynamic_scaler() for name, opt in self.opts.items()}
        if any(sc is None for sc in scalers.values()):
            return None
        return {name: sc.state_dict() for name, sc in scalers.items()}

    def load_state_dict(self, sd):
        for name, opt in self.opts.items():
            sc = opt.dynamic_scaler()
            if sc is not None and name in sd:
                sc.load_state_dict(sd[name])


class _Averaged:
    """Checkpoint entry "averaged": {agent: {"decay": d, "state": {parameter name as in the module's state_dict: average}}} for
    the agents that keep an average.  Absent when none does, so the file then has the reference's keys only.  Loading restores
    the values; the decay stays the one the trainer was built with."""

    def __init__(self, trainer):
        self.agents = trainer._agents
        self.loaded = set()   # the agents the most recent load_state_dict() restored (resume_from_ckpt resets the others)

    def state_dict(self):
        out = {}
        for name, net, opt in self.agents():
            if opt.averaging is not None:
                avg = opt.average_state()
                out[name] = {"decay": opt.averaging,
                             "state": {k: avg[p].detach().clone() for k, p in net.named_parameters() if p in avg}}
        return out or None

    def load_state_dict(self, sd):
        for name, net, opt in self.agents():
            if opt.averaging is not None and name in sd:
                params = dict(net.named_parameters())
                opt.load_average({params[k]: v for k, v in sd[name]["state"].items()})
                self.loaded.add(name)


class _Optimism:
    """Checkpoint entry "optimism": {agent: {"omega": w, "state": {parameter name as in the module's state_dict: previous direction}}}
    for the agents that step optimistically.  Absent when none does, so the file then has the reference's keys only.  Loading
    restores the directions; omega stays the one the trainer was built with."""

    def __init__(self, trainer):
        self.agents = trainer._agents
        self.loaded = set()   # the agents the most recent load_state_dict() restored (resume_from_ckpt primes the others)

    def state_dict(self):
        out = {}
        for name, net, opt in self.agents():
            if opt.optimism is not None:
                prev = opt.optimism_state()
                out[name] = {"omega": opt.optimism,
                             "state": {k: prev[p].detach().clone() for k, p in net.named_parameters() if p in prev}}
        return out or None

    def load_state_dict(self, sd):
        for name, net, opt in self.agents():
            if opt.optimism is not None and name in sd:
                params = dict(net.named_parameters())
                opt.load_optimism({params[k]: v for k, v in sd[name]["state"].items()})
                self.loaded.add(name)


class GIMImgTrainer(GimTrainerBase):
    IM_GROUPS = ("src_encoder", "env_encoder", "env_decoder", "img2img", "img_att", "env_noise_mapper")

    def __init__(self, outdir, m, n, k, authenticator, impersonator, au_lr, im_lr, env_noise_mapping_lr,
                 beta1=0., beta2=0.99, lr_milestones=(), lr_gamma=0.3, reg_param=10., remove_noise_mean=True,
                 im_optimism=None, au_optimism=None, im_ema_decay=None, au_ema_decay=None):
        super().__init__()
        self._init_agents(m, n, k, authenticator, impersonator, reg_param, remove_noise_mean)
        betas = (beta1, beta2)
        self.authenticator_opt = FusedAdam(self.authenticator.parameters(), lr=au_lr, betas=betas)
        # six parameter groups in the reference's order (their indices are part of the checkpoint format,
        # training/gim_img_trainer.py:52-58); only the noise mapper has a learning rate of its own
        groups = [(sub, env_noise_mapping_lr if sub == "env_noise_mapper" else im_lr) for sub in self.IM_GROUPS]
        self.impersonator_opt = FusedAdam([{"params": getattr(self.impersonator, sub).parameters(), "lr": lr} for sub, lr in groups],
                                          lr=im_lr, betas=betas)
        self.au_scheduler, self.im_scheduler = (self.get_lr_scheduler(optimizer=o, milestones=lr_milestones, gamma=lr_gamma)
                                                for o in (self.authenticator_opt, self.impersonator_opt))
        self._init_checkpoints(outdir)
        self.checkpoint_io.register_optional(loss_scalers=_LossScalers(authenticator_opt=self.authenticator_opt,
                                                                       impersonator_opt=self.impersonator_opt))
        self._init_averaging(im_ema_decay, au_ema_decay)
        self._init_optimism(im_optimism, au_optimism)

    def authenticator_forward(self, fake_sample, real_sample, si_sample, grad=True):
        ops.join_lanes()
        self._wants_input_grad(real_sample, si_sample)
        au = self.authenticator
        au.prefetch_spectral(3)  # si, real, fake: three calls of each encoder
        # same per-encoder call order as the reference (si, real, fake); the two encoders run on two streams
        (si_src, real_src, fake_src), (si_env, real_env, fake_env) = au.encode_samples([si_sample, real_sample, fake_sample])
        return self._discriminator_terms(
            au.dis(test_src=real_src, test_env=real_env, si_src=si_src, si_env=si_env),
            lambda: au.dis(test_src=fake_src, test_env=fake_env, si_src=si_src, si_env=si_env),
            real_sample, si_sample, fake_sample, grad)

    def impersonator_forward(self, leaked_sample, si_sample, z=None):
        fake_sample = self.impersonator(leaked_sample=leaked_sample, n=self.n, remove_noise_mean=self.remove_noise_mean, z=z)
        ops.join_lanes()   # a discriminator step still running on lane 1 (gim_step(defer_join=True)) owns the weights read next
        with _frozen(self.authenticator):
            auth_out = self.authenticator(test_sample=fake_sample, si_sample=si_sample)
        return self.gan_loss(dis_out=auth_out, target=1.), fake_sample, auth_out

    # ---- checkpoints (format: training_utils.CheckpointIO; file name as training/gim_img_trainer.py:158-172) ----
    def save(self, epoch):
        ops.join_lanes()   # the discriminator step of the last iteration may still be running on lane 1
        step = self.global_step
        print("\nSaving checkpoint...\n")
        self.checkpoint_io.save(global_step=step, last_epoch=epoch, filename="model_{:08}.pt".format(step))

    # ---- learning rates: MultiStepLR over both optimizers, stepped once per iteration by the caller loop ----
    def get_lr_scheduler(self, optimizer, milestones, gamma):
        return optim.lr_scheduler.MultiStepLR(optimizer=optimizer, milestones=list(milestones), gamma=gamma,
                                              last_epoch=self.global_step)

    def update_learning_rate(self):
        for sched in (self.au_scheduler, self.im_scheduler):
            if sched is not None:
                sched.step()

    @property
    def au_lr(self):
        return self.au_scheduler.get_last_lr()[0]

    @property
    def im_lr(self):
        return self.im_scheduler.get_last_lr()[0]

    @property
    def im_noise_mapping_lr(self):
        return self.im_scheduler.get_last_lr()[-1]
