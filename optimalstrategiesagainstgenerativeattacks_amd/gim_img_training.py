"""The optimisation-step protocol of the reference's ``training/gim_img_training.py``
(im_eval_step :76, au_eval_step :85, im_train_step :157, au_train_step :169) on the MI355X engine, plus a fused
convenience ``gim_step`` (= im_train_step then au_train_step, as train_epoch does at :225-239)."""
import contextlib
import itertools
import os

import torch
import torch.distributed as dist
from torch.utils.data import DataLoader
from tqdm import tqdm

from . import model_blocks as mb
from . import ops
from .training_logger import Logger
from .training_utils import DataParallelMock, EpisodeParallel, adjust_batch_size, get_device

_OVERLAP = os.environ.get("GIM_NO_STEP_OVERLAP") is None  # A/B switch


def _micro_batches(micro_batches, *tensors):
    """The checked number A of micro-batches of a step on these [B, ...] tensors (None entries are skipped).  ValueError for
    anything but an integer >= 1 that divides B - raised before the step touches the GPU."""
    A = micro_batches
    if isinstance(A, bool) or not isinstance(A, int):
        raise ValueError("micro_batches must be an integer >= 1, got %r" % (A,))
    if A < 1:
        raise ValueError("micro_batches must be >= 1, got %d" % A)
    for t in tensors:
        if t is not None and t.size(0) % A != 0:
            raise ValueError("a local batch of %d episodes cannot be cut into %d equal micro-batches" % (t.size(0), A))
    return A


def _micro_batch(sn, j, A, *tensors):
    """(context, slices) of micro-batch j of A: equal slices along dim 0, cut the way EpisodeParallel.shard cuts ranks, each a
    leaf of its own.  A == 1: the tensors themselves and a context that does nothing - the plain step.  Otherwise the context
    is sn's (mb.SNReplay): micro-batch 0 runs the spectral-norm power iterations, the others take its results."""
    if A == 1:
        return contextlib.nullcontext(), tensors
    out = []
    for t in tensors:
        per = None if t is None else t.size(0) // A
        out.append(None if t is None else t[j * per:(j + 1) * per].detach())
    return sn.micro_batch(j), tuple(out)


def _whole_batch_z(trainer, A, leaked_sample, z):
    """The latent noise of an accumulated generator pass that was given none: drawn here for the WHOLE batch, by the call the
    impersonator's forward makes, so that the slices see - and the generator consumes - the random numbers of the whole-batch step."""
    if A == 1 or z is not None:
        return z
    mod = trainer.module
    return torch.randn((leaked_sample.size(0), mod.n, mod.impersonator.style_dim), device=leaked_sample.device)


def _merged(outs, cat):
    """One return tuple from the tuples of the micro-batches: positions in `cat` hold per-episode tensors and are concatenated
    in batch order, the others hold means over the slice's episodes and become the mean over the (equal) slices: the mean over
    the whole batch.  Device work only."""
    if len(outs) == 1:
        return outs[0]
    return tuple(torch.cat(v, 0) if i in cat else torch.stack(v).mean(0) for i, v in enumerate(zip(*outs)))


_IM_CAT, _AU_CAT = (1, 2), (6, 7, 8)   # fake_sample, au_out; pred_on_real, pred_on_fake, fake_sample


def im_eval_step(trainer, leaked_sample, si_sample, z=None, micro_batches=1):
    A = _micro_batches(micro_batches, leaked_sample, si_sample, z)
    trainer.module.impersonator.eval()
    z = _whole_batch_z(trainer, A, leaked_sample, z)
    sn, outs = mb.SNReplay(), []
    for j in range(A):
        ctx, (leaked, si, z_) = _micro_batch(sn, j, A, leaked_sample, si_sample, z)
        with ctx, torch.no_grad():
            loss, fake_sample, au_out = trainer.forward(mode='impersonator_forward', leaked_sample=leaked,
                                                        si_sample=si, **({} if z_ is None else {"z": z_}))
            loss = loss.mean()
        outs.append((loss.detach(), fake_sample.detach(), au_out.detach()))
    return _merged(outs, _IM_CAT)


def _au_outputs(out):
    (loss, loss_on_real, loss_on_fake, reg, out_on_real, out_on_fake, pred_on_real, pred_on_fake, fake_sample) = out
    return (loss.detach(), loss_on_real.detach().mean(), loss_on_fake.detach().mean(), reg.detach().mean(),
            out_on_real.detach().mean(), out_on_fake.detach().mean(),
            pred_on_real.detach(), pred_on_fake.detach(), fake_sample.detach())


def au_eval_step(trainer, real_sample, fake_sample, si_sample, micro_batches=1):
    A = _micro_batches(micro_batches, real_sample, fake_sample, si_sample)
    trainer.module.authenticator.eval()
    sn, outs = mb.SNReplay(), []
    for j in range(A):
        ctx, (real, fake, si) = _micro_batch(sn, j, A, real_sample, fake_sample, si_sample)
        with ctx, torch.no_grad():
            out = trainer.forward(mode='authenticator_forward', fake_sample=fake, real_sample=real, si_sample=si, grad=False)
            out = (out[0].mean(),) + tuple(out[1:])
        outs.append(_au_outputs(out))
    return _merged(outs, _AU_CAT)


def _backward(loss, opt):
    """loss.backward() - on the fp16 matrix path of (loss * S), S = ops.loss_scale() (the optimizer step un-scales: FusedAdam.step
    (grad_scale=1 / S)), so that the gradients the fp16 convolution kernels round stay inside fp16's precise range.  In dynamic
    mode S is the device scalar of `opt`'s LossScaler and the backward pass runs armed (ops.armed_backward): an overflow becomes an
    infinity that the optimizer step finds."""
    sc = opt.dynamic_scaler()   # None: static scale, or the fp32 matrix path
    s = ops.loss_scale()
    with ops.caller_thread_backward(), ops.armed_backward(sc):     # (the nodes' Python on this thread: 15-25 % less host time per step, see ops)
        if sc is not None:
            sc.scale_loss(loss).backward()
        elif s != 1.0:
            (loss * s).backward()
        else:
            loss.backward()


def _opt_step(opt, micro_batches=1):
    """The optimizer step behind _backward(loss, opt): un-scales by the static scale, or - dynamic mode - by the scaler's own.
    micro_batches = A: A backward passes have added into the bucket since zero_grad(); the one update takes their mean.  (The loss
    scale is the same for all A: the static one is a host constant, the dynamic one moves inside this call only - where an
    infinity left by ANY of the A passes makes the guarded kernel skip the update and halve the scale, once.)"""
    if opt.dynamic_scaler() is not None:
        opt.step(micro_batches=micro_batches)
    else:
        sc, opt.loss_scaler = opt.loss_scaler, None   # (a scaler left from dynamic mode keeps its state, unused)
        try:
            opt.step(grad_scale=1.0 / ops.loss_scale(), micro_batches=micro_batches)
        finally:
            opt.loss_scaler = sc


def im_train_step(trainer, leaked_sample, si_sample, z=None, micro_batches=1):
    """micro_batches = A > 1: ONE generator update from A forward / backward passes on equal slices of the batch (see gim_step)."""
    A = _micro_batches(micro_batches, leaked_sample, si_sample, z)
    opt = trainer.module.impersonator_opt
    trainer.module.impersonator.train()
    opt.zero_grad()
    z = _whole_batch_z(trainer, A, leaked_sample, z)
    sn, outs = mb.SNReplay(), []
    for j in range(A):
        ctx, (leaked, si, z_) = _micro_batch(sn, j, A, leaked_sample, si_sample, z)
        with ctx:
            loss, fake_sample, au_out = trainer.forward(mode='impersonator_forward', leaked_sample=leaked,
                                                        si_sample=si, **({} if z_ is None else {"z": z_}))
            loss = loss.mean()
            _backward(loss, opt)
        outs.append((loss.detach(), fake_sample.detach(), au_out.detach()))
    _opt_step(opt, A)
    return _merged(outs, _IM_CAT)


def au_train_step(trainer, real_sample, fake_sample, si_sample, micro_batches=1):
    """micro_batches = A > 1: ONE discriminator update from A forward / backward passes on equal slices of the batch (see gim_step)."""
    A = _micro_batches(micro_batches, real_sample, fake_sample, si_sample)
    opt = trainer.module.authenticator_opt
    trainer.module.authenticator.train()
    opt.zero_grad()
    sn, outs = mb.SNReplay(), []
    for j in range(A):
        ctx, (real, fake, si) = _micro_batch(sn, j, A, real_sample, fake_sample, si_sample)
        with ctx:
            out = trainer.forward(mode='authenticator_forward', fake_sample=fake, real_sample=real, si_sample=si)
            out = (out[0].mean(),) + tuple(out[1:])
            _backward(out[0], opt)
        outs.append(_au_outputs(out))
    _opt_step(opt, A)
    return _merged(outs, _AU_CAT)


def gim_step(trainer, leaked_sample, real_sample, si_sample, z=None, overlap=None, defer_join=False, micro_batches=1):
    """One training iteration on one episode batch: generator step then discriminator step on the fake
    sample produced with the pre-update generator (training/gim_img_training.py:225-239, n_au_steps=1).

    On the GPU the two steps overlap: the discriminator step depends on the generator's FORWARD only (the fake sample),
    not on its backward or update, and the generator's backward only reads the discriminator's weights.  So the
    discriminator step runs on its own stream (lane 1) next to the generator's backward, with two orderings kept:
    the discriminator's Adam update waits for the generator's backward (which reads those weights), and the caller's
    stream waits for the discriminator step at the end.  Results are those of the sequential protocol.
    defer_join=True additionally leaves the caller's stream un-joined at return, so that the generator part of the NEXT
    iteration's forward runs under the tail of this discriminator step; the join happens where the discriminator's weights
    or outputs are next needed (ops.join_lanes(): inside the trainer's forward modes, save(), and by callers before they read
    the returned discriminator statistics).
    overlap=False (or GIM_NO_STEP_OVERLAP=1) runs the two steps back to back; hipGraph capture does (a hipGraph replays
    parallel branches slower than eager streams run them: 234 vs 282 episodes/s).

    micro_batches = A > 1 - gradient accumulation: the same iteration on a batch that does not fit one pass.  The batch is cut into A
    equal slices (dim 0); each slice runs the generator's forward and backward and, on lane 1, the discriminator's; the gradients
    add up in the optimizers' buckets (zeroed once); each optimizer then makes ONE update with the bucket scaled by 1 / A - the
    step on the whole batch, since the networks have no BatchNorm and every loss is a mean over episodes.  The spectral-norm power
    iterations run in the first slice only (mb.SNReplay), learning-rate schedule, global step and Adam's counter move once.  Losses and
    mean outputs are returned as means over the slices, per-episode outputs concatenated; nothing is read back in between."""
    A = _micro_batches(micro_batches, leaked_sample, real_sample, si_sample, z)
    if overlap is None:
        overlap = _OVERLAP
    if not (overlap and leaked_sample.is_cuda):
        im = im_train_step(trainer, leaked_sample, si_sample, z=z, micro_batches=A)
        au = au_train_step(trainer, real_sample, im[1], si_sample, micro_batches=A)
        return im, au
    from .gim_img_models import lane_stream
    mod = trainer.module
    cur = torch.cuda.current_stream()
    dstream = lane_stream(leaked_sample.device, 1)
    sn, ims, aus = mb.SNReplay(), [], []

    ops.mark_phase("step start")
    mod.impersonator.train()
    mod.impersonator_opt.zero_grad()
    z = _whole_batch_z(trainer, A, leaked_sample, z)
    for j in range(A):
        last = j == A - 1
        ctx, (leaked, real, si, z_) = _micro_batch(sn, j, A, leaked_sample, real_sample, si_sample, z)
        with ctx:
            # generator: forward on the caller's stream
            loss, fake_sample, au_out = trainer.forward(mode='impersonator_forward', leaked_sample=leaked,
                                                        si_sample=si, **({} if z_ is None else {"z": z_}))
            loss = loss.mean()
            fake_d = fake_sample.detach()
            ops.mark_phase("G forward done")
            ops.stream_wait(dstream, cur)            # lane 1 forks here: everything up to the generator's forward is visible to it
            for t in (fake_d, real, si):
                t.record_stream(dstream)

            # generator: backward on the caller's stream (enqueued first: it is the longer dependency chain; enqueueing the discriminator's
            # FORWARD ahead of it - so that lane 1 starts ~8 ms of host time earlier - was measured 4 % SLOWER, 406 vs 423 episodes/s over
            # three alternating pairs on one box: lane 1's early kernels take the chip from the critical lane; profiles/r04_d_*)
            _backward(loss, mod.impersonator_opt)
            ops.mark_phase("G backward done")
            if last:
                gbwd_done = cur.record_event()
                # generator's Adam right away: nothing on lane 1 reads the generator's weights, and with several GPUs its gradient
                # all-reduce (the larger bucket, 246 MB) then runs under the discriminator step instead of after it
                _opt_step(mod.impersonator_opt, A)
                ops.mark_phase("G update done")
            ims.append((loss.detach(), fake_d, au_out.detach()))

            # discriminator step on lane 1 (a slice's passes: under this slice's generator backward and the next slice's forward)
            with torch.cuda.stream(dstream), ops.lane(1):
                ops.mark_phase("D start")
                if j == 0:
                    mod.authenticator.train()
                    mod.authenticator_opt.zero_grad()
                out = trainer.forward(mode='authenticator_forward', fake_sample=fake_d, real_sample=real, si_sample=si)
                out = (out[0].mean(),) + tuple(out[1:])
                ops.mark_phase("D forward done")
                _backward(out[0], mod.authenticator_opt)
                ops.mark_phase("D backward done")
                if last:
                    dstream.wait_event(gbwd_done)   # the generator's backward reads the weights this update overwrites
                    _opt_step(mod.authenticator_opt, A)
                    ops.mark_phase("D update done")
                aus.append(_au_outputs(out))
    im = _merged(ims, _IM_CAT)
    au = aus[0]
    if A > 1:
        with torch.cuda.stream(dstream):
            au = _merged(aus, _AU_CAT)
    if defer_join:
        ops.defer_join(dstream)
    else:
        ops.stream_wait(cur, dstream)
    for t in au:
        t.record_stream(cur)
    return im, au


# --------------------------------------------------------------------------------------------------------------------
# the caller loop (training/gim_img_training.py:24-74, 98-154, 186-354, 356-441)
# --------------------------------------------------------------------------------------------------------------------
def save_imgs(logger, img_sample, category, k, global_step):
    if logger is None:   # a rank other than 0 of a data-parallel job: it ran the forward (see train_epoch) and logs nothing
        return
    imgs_for_save = ((img_sample[0].clamp(-1, 1) + 1) / 2.0).cpu()
    logger.add_imgs(imgs=imgs_for_save, category=category, k=k, global_step=global_step)


def sample_and_save_imgs(device, logger, trainer, ds, ds_prefix, indices, dbg=False):
    with torch.no_grad():
        global_step = trainer.module.get_global_step()
        for idx in indices:
            data = ds[idx]
            leaked_sample = data["leaked_sample"].unsqueeze(0).to(device)
            fake_sample = trainer.forward(mode='impersonator_sample', leaked_sample=leaked_sample)
            cat = "{} imgs_{:04}".format(ds_prefix, idx)
            save_imgs(logger=logger, img_sample=leaked_sample, category=cat, k="leaked", global_step=global_step)
            save_imgs(logger=logger, img_sample=fake_sample, category=cat, k="impersonator", global_step=global_step)
            if dbg:
                save_imgs(logger=logger, img_sample=data["real_sample"].unsqueeze(0).to(device), category=cat, k="real", global_step=global_step)
                save_imgs(logger=logger, img_sample=data["si_sample"].unsqueeze(0).to(device), category=cat, k="si", global_step=global_step)


def _averages(trainer):
    """Does the wrapped trainer keep averaged agents (GimTrainerBase.averages)?  A trainer without the notion keeps none."""
    fn = getattr(trainer.module, "averages", None)
    return fn is not None and fn()


def sample_and_save_avg_imgs(device, logger, trainer, ds, ds_prefix, indices):
    """One more image row per sampled index, k="impersonator_avg": the averaged impersonator's sample (eval mode, trainer.averaged())."""
    with trainer.module.averaged():
        global_step = trainer.module.get_global_step()
        for idx in indices:
            leaked_sample = ds[idx]["leaked_sample"].unsqueeze(0).to(device)
            fake_sample = trainer.forward(mode='impersonator_sample', leaked_sample=leaked_sample)
            save_imgs(logger=logger, img_sample=fake_sample, category="{} imgs_{:04}".format(ds_prefix, idx), k="impersonator_avg",
                      global_step=global_step)


def _world():
    return (dist.get_rank(), dist.get_world_size()) if dist.is_initialized() else (0, 1)


def _batches(ds, batch_size, shuffle, num_workers, device):
    """(iterator of batch dicts on `device`, number of batches).  A dataset that batches on the GPU itself
    (data.EpisodeBank.gpu_batches) is used directly; anything else goes through the reference's DataLoader."""
    rank, world = _world()
    if hasattr(ds, "gpu_batches"):
        return ds.gpu_batches(batch_size, shuffle, drop_last=True, rank=rank, world=world), ds.num_batches(batch_size)
    loader = DataLoader(ds, batch_size=batch_size, shuffle=shuffle, num_workers=num_workers, drop_last=True)
    per = batch_size // world

    def it():
        for b in loader:
            yield {k_: (v[rank * per:(rank + 1) * per].to(device, non_blocking=True) if torch.is_tensor(v) else v) for k_, v in b.items()}
    return it(), len(loader)


def eval_step(device, trainer, ds, logger, batch_size, category_suffix=""):
    """training/gim_img_training.py:98-154: one pass over `ds` with both agents in eval mode; per-batch statistics stay
    on the device and are fetched once at the end.  category_suffix: appended to the scalars' category names (the pass on the
    averaged agents logs under "... (averaged)")."""
    keys = ("au_loss", "au_loss_on_real", "au_loss_on_fake", "au_out_on_real", "au_out_on_fake", "au_acc", "au_acc_on_real",
            "au_acc_on_fake", "im_loss")
    acc = {k_: [] for k_ in keys}
    global_step = trainer.module.get_global_step()
    batches, num_iters = _batches(ds, batch_size, False, 0, device)
    rank, _ = _world()
    for data_batch in tqdm(itertools.islice(batches, num_iters), total=num_iters, desc='Eval', disable=rank != 0):
        real_sample, leaked_sample, si_sample = data_batch["real_sample"], data_batch["leaked_sample"], data_batch["si_sample"]
        im_loss, fake_sample, _ = im_eval_step(trainer=trainer, leaked_sample=leaked_sample, si_sample=si_sample)
        (au_loss, au_loss_on_real, au_loss_on_fake, au_reg, au_out_on_real, au_out_on_fake, au_pred_on_real, au_pred_on_fake,
         fake_sample) = au_eval_step(trainer=trainer, real_sample=real_sample, fake_sample=fake_sample, si_sample=si_sample)
        au_acc_on_real = au_pred_on_real.to(torch.float).mean()
        au_acc_on_fake = torch.eq(au_pred_on_fake, 0).to(torch.float).mean()
        vals = (au_loss, au_loss_on_real, au_loss_on_fake, au_out_on_real, au_out_on_fake, 0.5 * (au_acc_on_real + au_acc_on_fake),
                au_acc_on_real, au_acc_on_fake, im_loss)
        for k_, v in zip(keys, vals):
            acc[k_].append(v.view(1))
    if not acc["au_loss"]:
        return
    means = torch.stack([torch.cat(acc[k_]).mean() for k_ in keys]).tolist()   # one device -> host transfer
    names = (('eval losses', 'dis loss'), ('eval losses', 'dis loss on real'), ('eval losses', 'dis loss on fake'),
             ('eval au out', 'au out on real'), ('eval au out', 'au out on fake'), ('eval accuracy', 'dis acc'),
             ('eval accuracy', 'dis acc on real'), ('eval accuracy', 'dis acc on fake'), ('eval losses', 'gen loss'))
    for (category, k_), v in zip(names, means):
        logger.add_scalar(category=category + category_suffix, k=k_, v=v, global_step=global_step)


def train_epoch(device, logger, epoch, trainer, train_ds, val_ds, train_batch_size, val_batch_size, num_workers,
                save_every, eval_every, save_imgs_every, train_eval_indices, val_eval_indices,
                tb_log_every=100, tb_log_enc_every=500, n_au_steps=1, dbg=False, micro_batches=1):
    """training/gim_img_training.py:186-354.  Same protocol and cadences; the generator step and the discriminator step of
    an iteration are issued through gim_step (overlapped on two streams) when the generator trains this iteration.  Nothing
    is fetched from the device between log points.  micro_batches = A: every iteration accumulates its gradients over A slices of
    the rank's batch (gim_step); an iteration stays one global step, one learning-rate step and one update per optimizer.
    A trainer that keeps averaged agents (im_ema_decay / au_ema_decay) adds, behind the existing calls: one image row
    "impersonator_avg" per sampled index at save_imgs_every and a second eval pass on the averaged agents at eval_every."""
    _micro_batches(micro_batches)
    if (train_batch_size // _world()[1]) % micro_batches != 0:
        raise ValueError("a local batch of %d episodes cannot be cut into %d equal micro-batches" % (train_batch_size // _world()[1], micro_batches))
    buf = {k_: [] for k_ in ("au_loss", "au_loss_on_real", "au_loss_on_fake", "au_reg", "au_out_on_real", "au_out_on_fake",
                             "au_pred_on_real", "au_pred_on_fake", "im_loss")}
    rank, _ = _world()
    batches, n_batches = _batches(train_ds, train_batch_size, True, num_workers, device)
    num_iters = min(50, n_batches) if dbg else n_batches
    mbs = {} if micro_batches == 1 else {"micro_batches": micro_batches}
    for data_batch in tqdm(itertools.islice(batches, num_iters), total=num_iters, desc='Training', disable=rank != 0):
        trainer.module.do_global_step()
        trainer.module.update_learning_rate()
        real_sample, leaked_sample, si_sample = data_batch["real_sample"], data_batch["leaked_sample"], data_batch["si_sample"]
        global_step = trainer.module.global_step

        if (global_step + 1) % n_au_steps == 0:
            (im_loss, fake_sample, _), au = gim_step(trainer, leaked_sample, real_sample, si_sample, defer_join=True, **mbs)
        else:
            im_loss, fake_sample, _ = im_eval_step(trainer=trainer, leaked_sample=leaked_sample, si_sample=si_sample, **mbs)
            au = au_train_step(trainer=trainer, real_sample=real_sample, fake_sample=fake_sample, si_sample=si_sample, **mbs)
        au_loss, au_loss_on_real, au_loss_on_fake, au_reg, au_out_on_real, au_out_on_fake, au_pred_on_real, au_pred_on_fake, fake_sample = au
        buf["im_loss"].append(im_loss.view(1))
        for k_, v in (("au_loss", au_loss), ("au_loss_on_real", au_loss_on_real), ("au_loss_on_fake", au_loss_on_fake),
                      ("au_reg", au_reg), ("au_out_on_real", au_out_on_real), ("au_out_on_fake", au_out_on_fake)):
            buf[k_].append(v.view(1))
        buf["au_pred_on_real"].append(au_pred_on_real.view(-1))
        buf["au_pred_on_fake"].append(au_pred_on_fake.view(-1))

        if global_step % tb_log_every == 0:
            ops.join_lanes()
            logger.add_scalar(category='lr', k='au', v=trainer.module.au_lr, global_step=global_step)
            logger.add_scalar(category='lr', k='im', v=trainer.module.im_lr, global_step=global_step)
            logger.add_scalar(category='lr', k='im_lm', v=trainer.module.im_noise_mapping_lr, global_step=global_step)
            acc_real = torch.cat(buf["au_pred_on_real"]).to(torch.float).mean()
            acc_fake = torch.eq(torch.cat(buf["au_pred_on_fake"]), 0).to(torch.float).mean()
            vals = [torch.cat(buf[k_]).mean() for k_ in ("au_loss", "au_loss_on_real", "au_loss_on_fake", "au_reg", "au_out_on_real",
                                                         "au_out_on_fake")] + [0.5 * (acc_real + acc_fake), acc_real, acc_fake,
                                                                               torch.cat(buf["im_loss"]).mean()]
            vals = torch.stack(vals).tolist()   # the only device -> host transfer of the log point
            names = (('train_losses', 'dis_loss'), ('train_losses', 'dis_loss_on_real'), ('train_losses', 'dis_loss_on_fake'),
                     ('train_losses', 'dis_reg'), ('train_au_out', 'au_out_on_real'), ('train_au_out', 'au_out_on_fake'),
                     ('train_accuracy', 'dis_acc'), ('train_accuracy', 'dis_acc_on_real'), ('train_accuracy', 'dis_acc_on_fake'),
                     ('train losses', 'gen loss'))
            for (category, k_), v in zip(names, vals):
                logger.add_scalar(category=category, k=k_, v=v, global_step=global_step)
            if ops.matrix_path() == "fp16" and ops.loss_scale_mode() == "dynamic":   # only then: the other modes' call stream stays as it is
                for agent, opt in (("au", trainer.module.authenticator_opt), ("im", trainer.module.impersonator_opt)):
                    st = opt.dynamic_scaler().state()
                    logger.add_scalar(category='loss_scale', k=agent, v=st["scale"], global_step=global_step)
                    logger.add_scalar(category='loss_scale', k=agent + '_skipped', v=st["skipped"], global_step=global_step)
            for k_ in buf:
                buf[k_] = []

        if global_step % tb_log_enc_every == 0:
            ops.join_lanes()
            with torch.no_grad():
                au = trainer.module.authenticator
                enc = {}
                for nm, smp in (("real", real_sample), ("si", si_sample), ("fake", fake_sample)):
                    enc[nm + "_src"] = au.src_encode_sample(smp)
                    enc[nm + "_env"] = au.env_encode_sample(smp)
                for kind in ("src", "env"):
                    for nm in ("real", "fake"):
                        d = torch.abs(enc[nm + "_" + kind].mean(1) - enc["si_" + kind].mean(1)).mean().item()
                        logger.add_scalar(category='train-au_%s_mean' % kind, k='abs[%s-si]' % nm, v=d, global_step=global_step)
                    for nm in ("real", "si", "fake"):
                        logger.add_scalar(category='train-au_%s_std' % kind, k=nm, v=mb.custom_std(enc[nm + "_" + kind]).mean().item(),
                                          global_step=global_step)

        if global_step % save_every == 0 and rank == 0:
            trainer.module.save(epoch=epoch)
        if global_step % save_imgs_every == 0:
            # EVERY rank runs these generator forwards (only rank 0 writes the images): the generator is in train mode here, as in
            # the reference, so each forward runs one spectral-norm power iteration per conv - a rank that skipped them would
            # carry different u / v buffers, hence different sigma, from then on
            lg = logger if rank == 0 else None
            sample_and_save_imgs(device=device, logger=lg, trainer=trainer, ds=train_ds, ds_prefix='train', indices=train_eval_indices, dbg=dbg)
            sample_and_save_imgs(device=device, logger=lg, trainer=trainer, ds=val_ds, ds_prefix='val', indices=val_eval_indices, dbg=dbg)
            if _averages(trainer):   # behind the train-mode samples, whose call stream and u / v effects stay as they are
                sample_and_save_avg_imgs(device=device, logger=lg, trainer=trainer, ds=train_ds, ds_prefix='train', indices=train_eval_indices)
                sample_and_save_avg_imgs(device=device, logger=lg, trainer=trainer, ds=val_ds, ds_prefix='val', indices=val_eval_indices)
        if global_step % eval_every == 0:
            eval_step(device=device, trainer=trainer, ds=val_ds, logger=logger, batch_size=val_batch_size)
            if _averages(trainer):
                with trainer.module.averaged():
                    eval_step(device=device, trainer=trainer, ds=val_ds, logger=logger, batch_size=val_batch_size,
                              category_suffix=" (averaged)")
    ops.join_lanes()


def train_gim_imgs(device_name, device_ids, outdir, train_ds, val_ds, authenticator, impersonator, m, n, k,
                   reg_param, remove_noise_mean, au_lr, im_lr, beta1, beta2, env_noise_mapping_lr, lr_gamma, milestones,
                   resume_from_ckpt, n_epochs, batch_size, num_workers, save_every, eval_every, save_imgs_every,
                   train_eval_indices, val_eval_indices, n_au_steps=1, dbg=False, micro_batches=1,
                   im_optimism=None, au_optimism=None, im_ema_decay=None, au_ema_decay=None):
    """training/gim_img_training.py:356-441.  micro_batches: see train_epoch.  im_ema_decay / au_ema_decay: keep an exponential moving
    average of the impersonator's / authenticator's weights (GIMImgTrainer; None = off).  im_optimism / au_optimism: omega in (0, 1] of
    the optimistic Adam step of the impersonator / authenticator (GIMImgTrainer; None = off).  `device_ids` keeps its meaning as "the GPUs of the job": with more than one,
    launch one process per GPU (torchrun) - each process builds the same trainer, takes its slice of every global batch
    and the two optimizers all-reduce their gradient buckets over RCCL (EpisodeParallel replaces nn.DataParallel)."""
    from .gim_img_trainer import GIMImgTrainer
    from .gim_img_models import stream_concurrency_check
    from .training_utils import pin_rank_to_cores
    _micro_batches(micro_batches)
    if dist.is_initialized() and not torch.cuda.is_initialized():
        pin_rank_to_cores()   # a core set per rank, before the first GPU call (the runtime's helper threads inherit it)
    device = get_device(device_type=device_name, device_ids=device_ids)
    stream_concurrency_check(device)   # warns when the engine's streams share a hardware queue (GPU_MAX_HW_QUEUES not in force)
    rank, world = _world()
    n_devices = world if dist.is_initialized() else 1
    assert batch_size % n_devices == 0

    logger = Logger(log_dir=os.path.join(outdir, 'logs'), img_dir=os.path.join(outdir, 'imgs'), tensorboard_dir=os.path.join(outdir, 'tb'))
    authenticator = authenticator.to(device)
    impersonator = impersonator.to(device)
    trainer = GIMImgTrainer(outdir=outdir, m=m, n=n, k=k, authenticator=authenticator, impersonator=impersonator,
                            au_lr=au_lr, im_lr=im_lr, env_noise_mapping_lr=env_noise_mapping_lr, beta1=beta1, beta2=beta2,
                            lr_milestones=milestones, lr_gamma=lr_gamma, reg_param=reg_param,
                            remove_noise_mean=remove_noise_mean, im_ema_decay=im_ema_decay, au_ema_decay=au_ema_decay,
                            im_optimism=im_optimism, au_optimism=au_optimism).to(device)
    if resume_from_ckpt:
        trainer.resume_from_ckpt(ckpt_path=resume_from_ckpt)
        trainer.to(device)
    if n_devices > 1:
        trainer = EpisodeParallel(trainer)
        trainer.broadcast_parameters()
    else:
        trainer = DataParallelMock(trainer)

    for ep in tqdm(range(n_epochs), "Epochs", disable=rank != 0):
        try:
            train_epoch(device=device, logger=logger, epoch=ep, trainer=trainer, train_ds=train_ds, val_ds=val_ds,
                        train_batch_size=adjust_batch_size(len(train_ds), batch_size, n_devices),
                        val_batch_size=adjust_batch_size(len(val_ds), batch_size, n_devices),
                        num_workers=num_workers, save_every=save_every, eval_every=eval_every, save_imgs_every=save_imgs_every,
                        train_eval_indices=train_eval_indices, val_eval_indices=val_eval_indices, n_au_steps=n_au_steps, dbg=dbg,
                        micro_batches=micro_batches)
        except KeyboardInterrupt:
            print("\nKeyboardInterrupt\nSaving checkpoint...\n")
            if rank == 0:
                trainer.module.save(ep)
            break
        except PermissionError as pe:
            print("\nPermissionError\n%s\nSaving checkpoint...\n" % pe)
            if rank == 0:
                trainer.module.save(ep)
            continue
    return trainer, logger
