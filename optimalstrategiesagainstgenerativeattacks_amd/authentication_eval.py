"""Inference path of the reference's ``authentication_eval`` on the engine:
``eval_gim_on_authentication.py:25-44,75-106`` (model -> agent wrappers), ``agents.py:16-58`` (Authenticator / Impersonator
agents, replay impersonator) and ``authentication_score.py:32-97`` (accuracy / ROC-AUC over a dataset).  Host-side glue
over the same modules: both networks run in eval mode under ``torch.no_grad()`` (no power iteration, sigma from the stored
u, v); batches come from ``data.EpisodeBank.gpu_batches`` or a DataLoader, and per-batch statistics stay on the device.

The baseline rows of the result table (``eval_gim_on_authentication.py:47-72,109-252``, ``agents.py:53-62``): siamese / ArcFace
authenticators (``baselines.py``), the random-source impersonator, the dispatchers by type name and ``eval_authentication_task``,
which writes the reference's CSV columns with the ``csv`` module."""
import csv
import itertools
import json
import os
import random

import numpy as np
import torch
from tqdm import tqdm

from . import ops
from .gim_img_training import _batches, _world
from .training_utils import get_latest_ckpt, load_args


def get_au_function(au):
    def au_model_func(test_sample, si_sample):
        with torch.no_grad():
            (au_si_src, au_test_src), (au_si_env, au_test_env) = au.encode_samples([si_sample, test_sample])
            out = au.dis(test_src=au_test_src, test_env=au_test_env, si_src=au_si_src, si_env=au_si_env)
        return out.detach()
    return au_model_func


def get_im_function(im, args_dict):
    def im_model_func(leaked_sample, n):
        with torch.no_grad():
            fake_sample = im.forward(leaked_sample=leaked_sample, n=n, remove_noise_mean=args_dict['remove_noise_mean'])
        return fake_sample.detach()
    return im_model_func


class Authenticator:
    def __init__(self, au_model_func, th=0.):
        self.au_model_func = au_model_func
        self.th = th

    def act(self, test_sample, si_sample):
        out = self.au_model_func(test_sample=test_sample, si_sample=si_sample)
        pred = torch.ge(out, self.th).to(torch.long)
        return out, pred


class Impersonator:
    def __init__(self, im_model_func):
        self.im_model_func = im_model_func

    def act(self, leaked_sample, n):
        return self.im_model_func(leaked_sample=leaked_sample, n=n)


def replay_impersonator(leaked_sample, n):
    m = leaked_sample.size(1)
    return torch.cat([leaked_sample[:, random.randrange(m)].unsqueeze(1) for _ in range(n)], dim=1)


def get_gim_authenticator(au):
    """agents.Authenticator around an engine authenticator (eval mode)."""
    au.eval()
    return Authenticator(get_au_function(au))


def get_gim_impersonator(im, args_dict):
    im.eval()
    return Impersonator(get_im_function(im, args_dict))


def comp_acc(pred_on_real, pred_on_fake):
    assert len(pred_on_real.size()) == 1 and len(pred_on_fake.size()) == 1
    assert pred_on_real.size(0) == pred_on_fake.size(0)
    acc_on_real = pred_on_real.to(torch.float).mean()
    acc_on_fake = torch.eq(pred_on_fake, 0).to(torch.float).mean()
    return 0.5 * (acc_on_real + acc_on_fake), acc_on_fake, acc_on_real


def roc_auc(y_true, y_score):
    """Area under the ROC curve = Mann-Whitney U statistic with mid-ranks for ties (sklearn.metrics.roc_auc_score)."""
    y_true = np.asarray(y_true).astype(bool)
    y_score = np.asarray(y_score, dtype=np.float64)
    order = np.argsort(y_score, kind="mergesort")
    ranks = np.empty(len(y_score), dtype=np.float64)
    s = y_score[order]
    i = 0
    while i < len(s):
        j = i
        while j + 1 < len(s) and s[j + 1] == s[i]:
            j += 1
        ranks[order[i:j + 1]] = 0.5 * (i + j) + 1.0
        i = j + 1
    n_pos, n_neg = int(y_true.sum()), int((~y_true).sum())
    return float((ranks[y_true].sum() - n_pos * (n_pos + 1) / 2.0) / (n_pos * n_neg))


def _roc_record_host(pos, neg):
    """The eight words of gim_roc_calibrate (include/gim_hip.h) for the NaN-free candidates [pos; neg], sort-based in fp64 on the
    host; the last word is the chosen score itself, not its bit pattern."""
    n_pos, n_neg = len(pos), len(neg)
    cand = np.concatenate([pos, neg])
    sp, sn = np.sort(pos), np.sort(neg)
    p0 = n_pos - np.searchsorted(sp, cand, side="left")          # positives >= c
    p1 = np.searchsorted(sn, cand, side="left")                  # negatives < c
    p2 = np.searchsorted(sn, cand, side="right") - p1            # negatives == c
    key = p0.astype(np.int64) * n_neg + p1.astype(np.int64) * n_pos
    best = np.flatnonzero(key == key.max())
    idx = int(best[cand[best] == cand[best].max()][0])           # the largest value with the best key, its first occurrence
    return [int(p1[:n_pos].sum()), int(p2[:n_pos].sum()), int(key[idx]), idx, int(p0[idx]), int(p1[idx]), 0, float(cand[idx])]


def _roc_stats(record, th, n_pos, n_neg):
    """The dict of roc_statistics from the record's integers (fp64 on the host) and the chosen score."""
    if record[6]:
        raise ValueError("roc_statistics: %d of the scores are NaN" % record[6])
    return {"auc": (record[0] + 0.5 * record[1]) / (n_pos * n_neg), "th": float(th),
            "balanced_acc": record[2] / (2 * n_pos * n_neg), "acc_on_real": record[4] / n_pos, "acc_on_fake": record[5] / n_neg,
            "n_real": n_pos, "n_fake": n_neg}


def _score_sets(out_on_real, out_on_fake):
    sets = []
    for name, v in (("out_on_real", out_on_real), ("out_on_fake", out_on_fake)):
        v = v.detach().reshape(-1) if torch.is_tensor(v) else np.asarray(v, dtype=np.float64).reshape(-1)
        if len(v) == 0:
            raise ValueError("roc_statistics: %s is empty" % name)
        sets.append(v)
    return sets


def roc_statistics_host(out_on_real, out_on_fake):
    """roc_statistics in numpy / fp64 on the host: the CPU path, and the reference the kernels are tested against."""
    pos, neg = (np.asarray(v.cpu().numpy() if torch.is_tensor(v) else v, dtype=np.float64)
                for v in _score_sets(out_on_real, out_on_fake))
    n_nan = int(np.isnan(pos).sum() + np.isnan(neg).sum())
    if n_nan:
        raise ValueError("roc_statistics: %d of the scores are NaN" % n_nan)
    record = _roc_record_host(pos, neg)
    return _roc_stats(record, record[7], len(pos), len(neg))


def roc_statistics(out_on_real, out_on_fake):
    """ROC statistics of the scores on real sets (positives) against the scores on fake sets (negatives), and the operating point
    a threshold calibration takes from them.  For every score c as a candidate threshold of the rule "accept when score >= c":
    tp(c) = #{real >= c}, tn(c) = #{fake < c}.  Returns a dict of Python floats / ints:
      auc          (#{(r, f) : f < r} + #{(r, f) : f == r} / 2) / (n_real n_fake) - equal to roc_auc bit for bit;
      th           the candidate with the largest balanced accuracy; among several the largest score (reject when in doubt);
      balanced_acc (tp / n_real + tn / n_fake) / 2 at th (>= 0.5), acc_on_real = tp / n_real (> 0), acc_on_fake = tn / n_fake;
      n_real, n_fake.
    th is one of the scores themselves, so `score >= th` reproduces acc_on_real / acc_on_fake exactly.  CUDA tensors are counted
    on the device (ops.roc_record: exact integer counts, one host read of eight words), anything else by roc_statistics_host; the
    two give the same dict.  An empty score set or a NaN score raises ValueError."""
    pos, neg = _score_sets(out_on_real, out_on_fake)
    if not (torch.is_tensor(pos) and torch.is_tensor(neg) and pos.is_cuda and neg.is_cuda):
        return roc_statistics_host(pos, neg)
    record, _ = ops.roc_record(pos, neg)
    th = np.array([record[7]], dtype=np.uint32).view(np.float32)[0]
    return _roc_stats(record, th, pos.numel(), neg.numel())


def collect_scores(device, ds, batch_size, num_workers, authenticator, impersonator, dbg=False):
    """The batch loop of authentication_score.py:45-97: the authenticator's outputs and decisions on every real set of `ds` and on
    the impersonator's answer to its leaked set.  -> (out_on_real, out_on_fake, pred_on_real, pred_on_fake), 1-D, on the device."""
    outs = {"or": [], "of": [], "pr": [], "pf": []}
    batches, n_batches = _batches(ds, batch_size, True, num_workers, device)
    num_iters = min(1000, n_batches) if dbg else n_batches
    rank, _ = _world()
    for data_batch in tqdm(itertools.islice(batches, num_iters), total=num_iters, desc='Eval Authentication', disable=rank != 0):
        real_sample, leaked_sample, si_sample = data_batch["real_sample"], data_batch["leaked_sample"], data_batch["si_sample"]
        n = real_sample.size(1)
        out_on_real, pred_on_real = authenticator.act(test_sample=real_sample, si_sample=si_sample)
        fake_sample = impersonator.act(leaked_sample=leaked_sample, n=n)
        out_on_fake, pred_on_fake = authenticator.act(test_sample=fake_sample, si_sample=si_sample)
        for k_, v in (("or", out_on_real), ("of", out_on_fake), ("pr", pred_on_real), ("pf", pred_on_fake)):
            outs[k_].append(v.view(-1).detach())
    return tuple(torch.cat(outs[k_]) for k_ in ("or", "of", "pr", "pf"))


def eval_authenticator_and_impersonator(device, ds, batch_size, num_workers, authenticator, impersonator, dbg=False):
    """authentication_score.py:45-97: accuracy (total, on fake, on real) and ROC-AUC of `authenticator` against `impersonator`."""
    out_on_real, out_on_fake, pred_on_real, pred_on_fake = collect_scores(device, ds, batch_size, num_workers, authenticator,
                                                                          impersonator, dbg=dbg)
    acc, acc_on_fake, acc_on_real = comp_acc(pred_on_real=pred_on_real, pred_on_fake=pred_on_fake)
    y_true = torch.cat([torch.ones_like(out_on_real), torch.zeros_like(out_on_fake)]).cpu().numpy()
    y_score = torch.cat([out_on_real, out_on_fake]).cpu().numpy()
    return acc, acc_on_fake, acc_on_real, roc_auc(y_true, y_score)


# ------------------------------------------------------------------------------------------------------
# baseline authenticators, random-source impersonator, the result table
# ------------------------------------------------------------------------------------------------------
def _flat_sets(sample):
    """[B, t, C, H, W] -> ([B * t, C, H, W], B, t)."""
    B, t = sample.shape[:2]
    return sample.reshape(B * t, *sample.shape[2:]), B, t


def get_siamese_au_function(model):
    """Mean embedding of the test set against mean embedding of the source-information set; both sets go through the embedding
    net in ONE pass."""
    def au_model_func(test_sample, si_sample):
        model.train(mode=False)
        with torch.no_grad():
            si, B, k = _flat_sets(si_sample)
            test, _, n = _flat_sets(test_sample)
            emb = model.encode(torch.cat([si, test], 0))
            si_emb = ops.mean_dim1(emb[:B * k].view(B, k, -1))
            test_emb = ops.mean_dim1(emb[B * k:].view(B, n, -1))
            logits = model.classify(si_emb, test_emb)
        return logits.squeeze().detach()
    return au_model_func


def get_arcface_au_function(arcface):
    """ArcFace score of the MEAN IMAGE of the test set against the mean image of the source-information set."""
    def au_model_func(test_sample, si_sample):
        arcface.train(mode=False)
        with torch.no_grad():
            img = test_sample.shape[2:]
            x1 = ops.mean_dim1(ops._req(test_sample, "test_sample").flatten(2)).view(-1, *img)
            x2 = ops.mean_dim1(ops._req(si_sample, "si_sample").flatten(2)).view(-1, *img)
            score, _ = arcface.predict(x1=x1, x2=x2)
        return score.detach()
    return au_model_func


def rand_source_impersonator(leaked_sample, n, gim_ds):
    """Per batch element the real sample of a randomly drawn example of the dataset (another source, most of the time)."""
    rows = [gim_ds[random.randint(0, len(gim_ds) - 1)]["real_sample"] for _ in range(leaked_sample.size(0))]
    fake = torch.stack([torch.as_tensor(r) for r in rows], dim=0)
    assert fake.size(1) == n, "the dataset's real sets have %d elements, %d asked for" % (fake.size(1), n)
    return fake.to(leaked_sample.device)


def get_siamese_authenticator(device, ckpt_path, args_dict):
    from .baselines import ProtonetEmbeddingNet, SiameseNet
    net = ProtonetEmbeddingNet(inp_n_channels=1, inp_img_size=32)      # the reference evaluates the siamese baseline on Omniglot only
    siamese = SiameseNet(net, net.embedding_dim)
    siamese.load_state_dict(torch.load(ckpt_path, map_location='cpu')['model'], strict=True)
    return Authenticator(get_siamese_au_function(siamese.to(device)), th=args_dict.get('th', 0.))


def get_arcface_authenticator(device, ckpt_path, args_dict):
    from .baselines import ArcFace, Backbone
    sd = torch.load(ckpt_path, map_location='cpu')['arcface']
    a = args_dict
    backbone = Backbone(a['num_layers'], a['dropout'], 'ir_se', a['img_size'], a['img_channels'])
    arcface = ArcFace(backbone, a['emb_dim'], n_classes=sd['head.kernel'].size(-1), th=a['th'])   # the class count is the head's width
    arcface.load_state_dict(sd, strict=True)
    return Authenticator(get_arcface_au_function(arcface.to(device)), th=arcface.th)


def _gim_state(ckpt_path, agent, averaged):
    """The state dict of `agent` in a GIM checkpoint; averaged: with the parameters of its "averaged" entry laid over it (the
    spectral-norm u, v stay the live ones).  KeyError when the run kept no average of that agent."""
    payload = torch.load(ckpt_path, map_location='cpu')
    sd = payload[agent]
    if averaged:
        entry = payload.get('averaged') or {}
        if agent not in entry:
            raise KeyError("checkpoint %s has no averaged %s" % (ckpt_path, agent))
        sd = dict(sd)
        sd.update(entry[agent]['state'])
    return sd


def _gim_authenticator_from_ckpt(device, ckpt_path, args_dict, averaged=False):
    from .gim_img_models import get_au
    au = get_au(img_size=args_dict['img_size'], img_channels=args_dict['img_channels'], style_dim=args_dict['style_dim'])
    au.load_state_dict(_gim_state(ckpt_path, 'authenticator', averaged))
    agent = get_gim_authenticator(au.to(device))
    agent.model = au
    return agent


def _gim_impersonator_from_ckpt(device, ckpt_path, args_dict, averaged=False):
    from .gim_img_models import get_im
    im = get_im(img_size=args_dict['img_size'], img_channels=args_dict['img_channels'], style_dim=args_dict['style_dim'],
                use_img_att=args_dict['use_img_att'], num_env_noise_layers=args_dict['num_env_noise_layers'])
    im.load_state_dict(_gim_state(ckpt_path, 'impersonator', averaged))
    agent = get_gim_impersonator(im.to(device), args_dict)
    agent.model = im
    return agent


def get_authenticator(device, au_type, ckpt_path, args_dict, averaged=False):
    """averaged: the GIM authenticator on its averaged weights (checkpoint entry "averaged"); the baselines keep none."""
    makers = {'gim': _gim_authenticator_from_ckpt, 'siamese': get_siamese_authenticator, 'arcface': get_arcface_authenticator}
    if au_type not in makers:
        raise ValueError("unsupported authenticator type %r (gim | siamese | arcface)" % (au_type,))
    if au_type == 'gim':
        return _gim_authenticator_from_ckpt(device, ckpt_path, args_dict, averaged=averaged)
    return makers[au_type](device, ckpt_path, args_dict)


def get_impersonator(device, im_type, ckpt_path, ds, args_dict, averaged=False):
    """averaged: the GIM impersonator on its averaged weights (checkpoint entry "averaged")."""
    if im_type == 'gim':
        return _gim_impersonator_from_ckpt(device, ckpt_path, args_dict, averaged=averaged)
    if im_type == 'replay':
        return Impersonator(replay_impersonator)
    if im_type == 'rnd_src':
        return Impersonator(lambda leaked_sample, n: rand_source_impersonator(leaked_sample, n, ds))
    raise ValueError("unsupported impersonator type %r (gim | replay | rnd_src)" % (im_type,))


def get_exp_args_from_dir(outdir, ckpt_dir, specific_model=None):
    """(checkpoint path, args dict) of an experiment directory: its latest checkpoint unless one is named."""
    ckpt_dir_path = os.path.join(outdir, ckpt_dir)
    path = get_latest_ckpt(ckpt_dir_path) if specific_model is None else os.path.join(ckpt_dir_path, specific_model)
    args_dict = load_args(outdir)
    if 'img_size' not in args_dict:
        args_dict['img_size'] = args_dict['target_img_size']
    return path, args_dict


def eval_game_for_pair(device, au_type, im_type, au_outdir, im_outdir, ds, batch_size, num_workers, ckpt_dir='ckpts',
                       specific_model=None, averaged=False):
    au_ckpt_path, au_args_dict = get_exp_args_from_dir(au_outdir, ckpt_dir, specific_model=specific_model)
    im_ckpt_path, im_args_dict = get_exp_args_from_dir(im_outdir, ckpt_dir, specific_model=specific_model)
    avg = {"averaged": True} if averaged else {}   # (passed only when asked for: the default call is what it was)
    au_agent = get_authenticator(device=device, au_type=au_type, ckpt_path=au_ckpt_path, args_dict=au_args_dict, **avg)
    im_agent = get_impersonator(device=device, im_type=im_type, ckpt_path=im_ckpt_path, ds=ds, args_dict=im_args_dict, **avg)
    acc, acc_on_fake, acc_on_real, auc = eval_authenticator_and_impersonator(
        device=device, ds=ds, batch_size=batch_size, num_workers=num_workers, authenticator=au_agent, impersonator=im_agent)
    return float(acc), float(acc_on_fake), float(acc_on_real), float(auc)


TABLE_COLUMNS = ('au_type', 'im_type', 'ds_root', 'gim_exp_dir', 'm', 'n', 'k', 'acc', 'acc_on_fake', 'acc_on_real', 'auc')


def eval_authentication_task(device, ds, m, n, k, batch_size, num_workers, gim_exp_dir, csv_file_path, specific_model=None,
                             baseline_exp_dir=None, baseline_type=None, averaged=False):
    """The result table: authenticator gim (and the baseline, if one is named) against impersonators gim, replay, rnd_src -
    one CSV row each, in that order.  Returns the rows.  averaged: the GIM agents run on their averaged weights."""
    out_dir = os.path.dirname(csv_file_path)
    if out_dir and not os.path.isdir(out_dir):
        os.makedirs(out_dir)
    rows = []
    for au_type in (['gim'] if baseline_type is None else ['gim', baseline_type]):
        for im_type in ('gim', 'replay', 'rnd_src'):
            print("running {} vs. {}".format(au_type, im_type))
            acc, acc_on_fake, acc_on_real, auc = eval_game_for_pair(
                device=device, au_type=au_type, im_type=im_type, au_outdir=gim_exp_dir if au_type == 'gim' else baseline_exp_dir,
                im_outdir=gim_exp_dir, ds=ds, batch_size=batch_size, num_workers=num_workers, specific_model=specific_model,
                **({"averaged": True} if averaged else {}))
            rows.append(dict(zip(TABLE_COLUMNS, (au_type, im_type, getattr(ds, "root", ""), gim_exp_dir, m, n, k,
                                                 acc, acc_on_fake, acc_on_real, auc))))
            print({c: rows[-1][c] for c in ('au_type', 'im_type', 'acc', 'acc_on_fake', 'acc_on_real')})
    with open(csv_file_path, 'w', newline='') as f:
        wr = csv.DictWriter(f, fieldnames=TABLE_COLUMNS)
        wr.writeheader()
        wr.writerows(rows)
    return rows


# ------------------------------------------------------------------------------------------------------
# calibrating a baseline's decision threshold
# ------------------------------------------------------------------------------------------------------
def calibrate_threshold(authenticator, device, ds, batch_size, num_workers, impersonator=None):
    """Sets authenticator.th to the threshold of the largest balanced accuracy (roc_statistics) on the real sets of `ds` against
    `impersonator` - by default the random-source impersonator over `ds`, the table's rnd_src row: other identities are what a
    verification threshold separates.  Returns the statistics."""
    if impersonator is None:
        impersonator = get_impersonator(device=device, im_type='rnd_src', ckpt_path=None, ds=ds, args_dict=None)
    out_on_real, out_on_fake, _, _ = collect_scores(device, ds, batch_size, num_workers, authenticator, impersonator)
    stats = roc_statistics(out_on_real, out_on_fake)
    authenticator.th = stats['th']
    return stats


def calibrate_baseline(device, baseline_type, baseline_exp_dir, ds, batch_size, num_workers=0, specific_model=None, ckpt_dir='ckpts'):
    """Calibrates the threshold of a trained baseline (siamese | arcface) on `ds` - held-out data, not the training set - and
    stores it in the experiment's args.json, from where eval_authentication_task loads it: `th` becomes the calibrated value and
    `th_calibration` records {auc, balanced_acc, acc_on_real, acc_on_fake, n_real, n_fake, ds_root, ckpt}; every other key is
    kept.  The file is replaced atomically.  Returns the statistics of calibrate_threshold."""
    if baseline_type not in ('siamese', 'arcface'):
        raise ValueError("unsupported baseline type %r (siamese | arcface)" % (baseline_type,))
    ckpt_path, args_dict = get_exp_args_from_dir(baseline_exp_dir, ckpt_dir, specific_model=specific_model)
    au_agent = get_authenticator(device=device, au_type=baseline_type, ckpt_path=ckpt_path, args_dict=args_dict)
    stats = calibrate_threshold(au_agent, device, ds, batch_size, num_workers)
    args = load_args(baseline_exp_dir)                     # the file as written, without the keys get_exp_args_from_dir derives
    args['th'] = stats['th']
    args['th_calibration'] = dict({k_: stats[k_] for k_ in ('auc', 'balanced_acc', 'acc_on_real', 'acc_on_fake', 'n_real', 'n_fake')},
                                  ds_root=getattr(ds, "root", ""), ckpt=os.path.basename(ckpt_path))
    path = os.path.join(baseline_exp_dir, "args.json")
    tmp = path + ".tmp.%d" % os.getpid()
    with open(tmp, "w") as f:
        json.dump(args, f)
    os.replace(tmp, path)
    return stats
