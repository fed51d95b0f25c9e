"""Worker of tests/test_gpu_baseline_dp.py (one child process per rank, both ranks on the one card, gloo between them):
    baseline_dp_worker.py <siamese | arcface | loop> <rank> <world> <port> <out_dir>
Runs the protocol of the single-process golden tests with every rank on its slice of the batch and writes what the parent asserts:
<out_dir>/result<rank>.pt (everything in GLOBAL row order, gradients as the all-reduced bucket / world; the parent reads rank 0's) and
<out_dir>/state<rank>.pt (the rank's final state dict)."""
import datetime
import json
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import arcface_fill as af  # noqa: E402
from tests import baseline_fill as bf  # noqa: E402
from tests import siamese_fill as sf  # noqa: E402
from tests.helpers import GOLDEN  # noqa: E402


def _at(t, idx):
    return t.detach().reshape(-1)[torch.from_numpy(idx).to(t.device)].double().cpu()


def _global_rows(sync, t):
    """[world, B_local, ...] gathered in rank order -> [B, ...] on the host."""
    g = sync.all_gather(t.detach().contiguous())
    return g.reshape(-1, *t.shape[1:]).cpu()


def _rank_mean(sync, v):
    return float(sync.all_reduce_(v.detach().clone().view(1)) / sync.world)


def _slice(B, rank, world):
    per = B // world
    return rank * per, (rank + 1) * per


def siamese(rank, world, dev, out_dir):
    from optimalstrategiesagainstgenerativeattacks_amd import baselines as bl
    from optimalstrategiesagainstgenerativeattacks_amd.baseline_training import SiameseTrainer
    with open(os.path.join(GOLDEN, "baseline_keys.json")) as f:
        keys = json.load(f)["keys"][sf.CFG]
    enc = bl.ProtonetEmbeddingNet(1, 32)
    model = bl.SiameseNet(enc, enc.embedding_dim)
    model.load_state_dict(bf.filled_state(keys, sf.PROTO_TAG, torch.float32), strict=True)
    model = model.to(dev)
    res = {"init": {k: v.detach().cpu().clone() for k, v in model.named_parameters()}}
    tr = SiameseTrainer(model, lr=sf.LR)       # the default sync: torch.distributed's default group
    sync = tr.sync
    assert sync is not None and (sync.rank, sync.world) == (rank, world)
    lo, hi = _slice(sf.PROTO_B, rank, world)
    n_pos = min(max(sf.PROTO_N_POS - lo, 0), hi - lo)
    res["n_pos"] = [int(v) for v in _global_rows(sync, torch.tensor([float(n_pos)], device=dev))]
    for it in range(sf.PROTO_ITERS):
        x1, x2 = (bf.images("%s%s/it%d" % (sf.PROTO_TAG, nm, it), (sf.PROTO_B, 1, 32, 32), torch.float32)[lo:hi].to(dev) for nm in ("x1", "x2"))
        loss, _ = tr.train_step(x1, x2, n_pos)
        res["it%d/logits" % it] = _global_rows(sync, tr.last_logits)
        res["it%d/loss" % it] = _rank_mean(sync, loss)
        if it == 0:
            for k, p in model.named_parameters():
                res["grad/" + k] = (p.grad / world).cpu()
        for k, v in model.state_dict().items():
            if k.endswith(("running_mean", "running_var", "num_batches_tracked")):
                res["it%d/%s" % (it, k)] = v.detach().cpu().clone()
    for k, p in model.named_parameters():
        res["final/" + k] = p.detach().cpu().clone()
    return res, tr.state_dict()["model"]


def arcface(rank, world, dev, out_dir):
    from optimalstrategiesagainstgenerativeattacks_amd import baselines as bl
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    from optimalstrategiesagainstgenerativeattacks_amd.baseline_training import ArcFaceTrainer
    assert ops.deterministic(), "run with GIM_DETERMINISTIC=1"
    model = bl.ArcFace(bl.Backbone(af.NUM_LAYERS, 0.0, 'ir_se', af.IMG_SIZE, af.IMG_CHANNELS), af.EMB_DIM, af.PROTO_CLASSES)
    model.load_state_dict(bf.filled_state(af.keys(af.PROTO_CLASSES), af.PROTO_TAG, torch.float32), strict=True)
    model = model.to(dev)
    tr = ArcFaceTrainer(model, lr=af.PROTO_LR)
    sync = tr.sync
    assert sync is not None and (sync.rank, sync.world) == (rank, world)
    lo, hi = _slice(af.PROTO_B, rank, world)
    label = torch.from_numpy(af.proto_labels()[lo:hi]).to(dev)
    res = {"names": [k for k, _ in model.named_parameters()]}
    for it in range(af.PROTO_ITERS):
        x = torch.from_numpy(af.proto_images(it)[lo:hi]).float().to(dev)
        if it == 0:
            before = {k: _at(p, af.delta_index(p.numel())) for k, p in model.named_parameters()}
        loss, _ = tr.train_step(x, label, it)
        res["it%d/emb" % it] = _global_rows(sync, tr.last_emb)
        res["it%d/logits" % it] = _global_rows(sync, tr.last_logits)
        res["it%d/loss" % it] = _rank_mean(sync, loss)
        sd = model.state_dict()
        for bn in af.RUNNING:
            for leaf in ("running_mean", "running_var", "num_batches_tracked"):
                res["it%d/run/%s.%s" % (it, bn, leaf)] = sd["emb_model.%s.%s" % (bn, leaf)].detach().cpu().clone()
        if it == 0:
            for k, p in model.named_parameters():
                res["gradnorm/" + k] = float(p.grad.double().norm()) / world
                res["grad/" + k] = _at(p.grad, af.sample_index(p.numel())) / world
                res["delta/" + k] = _at(p, af.delta_index(p.numel())) - before[k]
    return res, tr.state_dict()["model"]


def loop(rank, world, dev, out_dir):
    """train_siamese to iteration 4, then a second call that resumes and goes on to 6; a checkpoint every 2."""
    import optimalstrategiesagainstgenerativeattacks_amd as G
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    assert ops.deterministic(), "run with GIM_DETERMINISTIC=1"
    imgs, offs = sf.separable_bank(per_class=10)
    bank = G.EpisodeBank(torch.from_numpy(imgs).to(dev), offs, 1, 3, 4, example_cnt_per_class=1, mirror=False, seed=5)
    exp = os.path.join(out_dir, "exp")
    logs = []
    for n_iters in (4, 6):
        log = G.Logger(log_dir=os.path.join(out_dir, "logs%d_%d" % (n_iters, rank)), img_dir=os.path.join(out_dir, "imgs%d_%d" % (n_iters, rank)))
        tr = G.train_siamese(dev, bank, exp, n_iters, batch_size=8, log_every=2, save_every=2, seed=4, logger=log)
        logs.append({k: list(v) for k, v in log.stats.get("siamese", {}).items()})
        assert tr.sync is not None and tr.sync.world == world
    return {"logs": logs}, tr.state_dict()["model"]


def main():
    mode, rank, world, port, out_dir = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5]
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", port
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))      # a lost peer ends this rank
    dev = torch.device("cuda:0")
    res, state = {"siamese": siamese, "arcface": arcface, "loop": loop}[mode](rank, world, dev, out_dir)
    torch.cuda.synchronize()
    torch.save(state, os.path.join(out_dir, "state%d.pt" % rank))
    res["logged_on_rank"] = rank
    torch.save(res, os.path.join(out_dir, "result%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
