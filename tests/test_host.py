"""CPU suite (no GPU): host logic of the product package, the C-ABI library's exports, and the
data-parallel sharding / gradient exchange over gloo with world_size 2."""
import ctypes
import os
import re
import sys
import tempfile

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from tests.helpers import load_keys  # noqa: E402


def test_state_dict_keys_match_reference():
    """Names, shapes and ORDER of every state-dict entry and parameter equal the reference's (captured by
    oracle/make_golden.py), incl. the spectral-norm weight_orig / weight_u / weight_v triple."""
    import optimalstrategiesagainstgenerativeattacks_amd as G
    for cfg in ("16_1_32", "32_1_512"):
        s, c, d = map(int, cfg.split("_"))
        ref = load_keys(cfg)
        au, im = G.get_au(s, c, d), G.get_im(s, c, d)
        assert [[k, list(v.shape)] for k, v in au.state_dict().items()] == ref["au"]
        assert [[k, list(v.shape)] for k, v in im.state_dict().items()] == ref["im"]
        assert [k for k, _ in au.named_parameters()] == ref["au_params"]
        assert [k for k, _ in im.named_parameters()] == ref["im_params"]
        groups = [len(list(getattr(im, g).parameters())) for g in
                  ("src_encoder", "env_encoder", "env_decoder", "img2img", "img_att", "env_noise_mapper")]
        assert groups == ref["im_groups"]


def test_conv_weights_are_stored_channels_last():
    import optimalstrategiesagainstgenerativeattacks_amd as G
    au = G.get_au(16, 1, 32)
    w = au.src_encoder.down_blocks[0].conv_r2.weight_orig
    assert w.shape == (32, 32, 3, 3) and w.permute(0, 2, 3, 1).is_contiguous()
    sd = {k: v.clone() for k, v in au.state_dict().items()}
    au.load_state_dict(sd)  # plain NCHW-contiguous checkpoints load; storage stays channels-last
    assert au.src_encoder.down_blocks[0].conv_r2.weight_orig.permute(0, 2, 3, 1).is_contiguous()


def test_trainer_host_protocol():
    import optimalstrategiesagainstgenerativeattacks_amd as G
    au, im = G.get_au(16, 1, 32), G.get_im(16, 1, 32)
    with tempfile.TemporaryDirectory() as td:
        tr = G.GIMImgTrainer(td, 1, 3, 4, au, im, au_lr=2e-3, im_lr=1e-3, env_noise_mapping_lr=1e-4,
                             lr_milestones=(2,), lr_gamma=0.5, reg_param=0.0)
        assert os.path.isdir(os.path.join(td, "ckpts"))
        assert tr.global_step == -1
        assert len(tr.impersonator_opt.param_groups) == 6 and len(tr.authenticator_opt.param_groups) == 1
        assert tr.impersonator_opt.param_groups[-1]["lr"] == 1e-4
        assert tr.authenticator_opt.param_groups[0]["betas"] == (0.0, 0.99)
        lrs = []
        for _ in range(3):
            tr.do_global_step()
            tr.update_learning_rate()
            lrs.append((tr.au_lr, tr.im_lr, tr.im_noise_mapping_lr, tr.global_step))
        # MultiStepLR built with last_epoch=-1 and stepped before the optimiser: counter = it + 1
        assert lrs == [(2e-3, 1e-3, 1e-4, 0), (1e-3, 5e-4, 5e-5, 1), (1e-3, 5e-4, 5e-5, 2)]
        with pytest.raises(ValueError):
            tr.forward(mode="nope")
        tr.save(epoch=3)
        path = os.path.join(td, "ckpts", "model_%08d.pt" % 2)
        ck = torch.load(path, weights_only=False)
        assert set(ck) == {"global_step", "last_epoch", "authenticator", "impersonator", "authenticator_opt", "impersonator_opt"}
        assert ck["global_step"] == {"global_step": 2} and ck["last_epoch"] == 3
        au2, im2 = G.get_au(16, 1, 32), G.get_im(16, 1, 32)
        tr2 = G.GIMImgTrainer(td, 1, 3, 4, au2, im2, 2e-3, 1e-3, 1e-4, reg_param=0.0)
        tr2.resume_from_ckpt(path)
        assert tr2.global_step == 2
        for (k, a), (_, b) in zip(au.state_dict().items(), au2.state_dict().items()):
            assert torch.equal(a, b), k


def test_no_cpu_compute_path():
    """The product must fail loudly without the GPU: no silent CPU fallback anywhere."""
    import optimalstrategiesagainstgenerativeattacks_amd as G
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    au = G.get_au(16, 1, 32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        au(torch.zeros(1, 2, 1, 16, 16), torch.zeros(1, 2, 1, 16, 16))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.linear(torch.zeros(2, 4), torch.zeros(3, 4), torch.zeros(3))
    opt = G.FusedAdam(au.parameters(), lr=1e-3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step()


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "optimalstrategiesagainstgenerativeattacks_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle", src, re.M), f
                assert "gim_oracle" not in src, f


def test_library_exports_every_header_symbol():
    from optimalstrategiesagainstgenerativeattacks_amd import _lib
    header = open(os.path.join(ROOT, "include", "gim_hip.h")).read()
    declared = set(re.findall(r"\b(gim_[a-z0-9_]+)\s*\(", header))
    declared -= {"gim_conv_shape"}
    assert len(declared) >= 30
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in sorted(declared):
        assert hasattr(lib, name), "libgim_hip.so does not export %s" % name
    assert declared == set(_lib.SIGNATURES) | {"gim_last_error"}, declared ^ (set(_lib.SIGNATURES) | {"gim_last_error"})
    assert lib.gim_version() >= 1


# ---------------------------------------------------------------------------------------------------
# data parallelism over episodes: gloo, world_size 2
# ---------------------------------------------------------------------------------------------------
def _dp_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, ROOT)
    from oracle import gim_oracle as go
    from optimalstrategiesagainstgenerativeattacks_amd.optim import all_reduce_grads_
    from optimalstrategiesagainstgenerativeattacks_amd.training_utils import EpisodeParallel
    from tests.helpers import episode, filled_sd
    keys = load_keys("16_1_32")
    au = filled_sd(keys["au"], "dp/au/")
    go.set_requires_grad(au)
    B, n, k = 4, 2, 3
    _, real, si, _ = episode("dp", B, 1, n, k, 1, 16, 32)
    fake = real.flip(0).contiguous()
    ep = EpisodeParallel(module=None)
    assert (ep.rank, ep.world_size) == (rank, world)
    real_l, fake_l, si_l = ep.shard(real, fake, si)
    assert real_l.shape[0] == B // world
    loss = go.authenticator_forward(au, fake_l, real_l, si_l, True, 0.0)[0].mean()  # local mean, as au_train_step does
    loss.backward()
    names = [kk for kk in au if go.is_param(kk)]
    flat = torch.cat([au[kk].grad.reshape(-1) for kk in names])
    scale = all_reduce_grads_(flat)
    flat = flat * scale
    if rank == 0:
        q.put((flat, [au[kk].detach().clone() for kk in ("src_encoder.down_blocks.0.conv_r1.weight_u",)]))
    dist.barrier()
    dist.destroy_process_group()


def test_episode_data_parallel_equals_big_batch_gloo():
    """Sharding the episode batch over 2 ranks + one all-reduce(sum) of the flat gradient bucket (scaled by
    1/world) equals the single-process gradient of the whole batch; spectral-norm buffers need no sync."""
    from oracle import gim_oracle as go
    from tests.helpers import episode, filled_sd, relerr
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    flat_dp, bufs = q.get(timeout=300)
    for p in procs:
        p.join(timeout=300)
        assert p.exitcode == 0
    keys = load_keys("16_1_32")
    au = filled_sd(keys["au"], "dp/au/")
    go.set_requires_grad(au)
    _, real, si, _ = episode("dp", 4, 1, 2, 3, 1, 16, 32)
    fake = real.flip(0).contiguous()
    go.authenticator_forward(au, fake, real, si, True, 0.0)[0].mean().backward()
    flat = torch.cat([au[kk].grad.reshape(-1) for kk in au if go.is_param(kk)])
    assert relerr(flat_dp, flat) < 1e-10
    assert relerr(bufs[0], au["src_encoder.down_blocks.0.conv_r1.weight_u"]) < 1e-12


def _broadcast_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, ROOT)
    from optimalstrategiesagainstgenerativeattacks_amd.training_utils import EpisodeParallel
    torch.manual_seed(100 + rank)      # the ranks start from DIFFERENT values
    mod = torch.nn.Module()
    mod.weight = torch.nn.Parameter(torch.randn(6, 3, 3, 3).contiguous(memory_format=torch.channels_last))    # a conv weight as the engine stores it
    mod.bias = torch.nn.Parameter(torch.randn(6))
    mod.register_buffer("weight_u", torch.randn(6))
    tensors = dict(mod.named_parameters(), **dict(mod.named_buffers()))
    before = {k: t._version for k, t in tensors.items()}
    strides = {k: t.stride() for k, t in tensors.items()}
    EpisodeParallel(mod).broadcast_parameters()
    q.put((rank, {k: t.detach().clone() for k, t in tensors.items()}, before, {k: t._version for k, t in tensors.items()},
           all(t.stride() == strides[k] and t.requires_grad == (k != "weight_u") for k, t in tensors.items())))
    dist.barrier()
    dist.destroy_process_group()


def test_broadcast_parameters_advances_version_counters_gloo():
    """EpisodeParallel.broadcast_parameters over 2 gloo ranks: both ranks end with rank 0's values, and every parameter's and
    buffer's _version has advanced on BOTH ranks - what the derived-weight cache (ops._WT_CACHE) keys on, so a broadcast behind
    a forward pass cannot leave re-laid-out copies of the old weights in use (a write through .data would: it is invisible)."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_broadcast_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict((r[0], r[1:]) for r in (q.get(timeout=300), q.get(timeout=300)))
    for p in procs:
        p.join(timeout=300)
        assert p.exitcode == 0
    torch.manual_seed(100)
    w0 = torch.randn(6, 3, 3, 3)
    b0, u0 = torch.randn(6), torch.randn(6)
    for rank in (0, 1):
        vals, before, after, layout_kept = got[rank]
        assert torch.equal(vals["weight"], w0) and torch.equal(vals["bias"], b0) and torch.equal(vals["weight_u"], u0), rank
        for k in vals:
            assert after[k] > before[k], (rank, k, before[k], after[k])
        assert layout_kept, rank


def test_logger_mirror_and_training_loop_cadence(tmp_path):
    """The caller loop of training/gim_img_training.py:186-354 on a stub trainer (no GPU): n_au_steps gating of the generator
    step, log / save / eval cadences keyed on global_step, one device->host fetch per log point, Logger round trip."""
    import optimalstrategiesagainstgenerativeattacks_amd as G
    from optimalstrategiesagainstgenerativeattacks_amd import gim_img_training as gt
    calls = []

    class StubTrainer:
        def __init__(self):
            self.global_step = -1
            self.au_lr, self.im_lr, self.im_noise_mapping_lr = 1e-4, 1e-4, 1e-6
            self.saved = []

        def do_global_step(self):
            self.global_step += 1

        def update_learning_rate(self):
            pass

        def get_global_step(self):
            return self.global_step

        def save(self, epoch):
            self.saved.append((epoch, self.global_step))

        class authenticator:   # encoding statistics are logged at global_step 0 (0 % tb_log_enc_every == 0)
            src_encode_sample = staticmethod(lambda smp: torch.zeros(2, 3, 4))
            env_encode_sample = staticmethod(lambda smp: torch.zeros(2, 3, 4))

    class Wrap:
        def __init__(self, m):
            self.module = m

    one = torch.ones(())
    au_ret = (one, one, one, one * 0, one, -one, torch.ones(2, 1, dtype=torch.bool), torch.zeros(2, 1, dtype=torch.bool), torch.zeros(2))
    orig = (gt.gim_step, gt.im_eval_step, gt.au_train_step, gt.au_eval_step)
    orig_std = gt.mb.custom_std
    gt.mb.custom_std = lambda x: x.std(1)
    gt.gim_step = lambda tr, l, r, s, z=None, overlap=None, defer_join=False: (calls.append(("G+D", tr.module.global_step)), ((one, torch.zeros(2), one), au_ret))[1]
    gt.im_eval_step = lambda trainer, leaked_sample, si_sample, z=None: (calls.append(("Geval", trainer.module.global_step)), (one, torch.zeros(2), one))[1]
    gt.au_train_step = lambda trainer, real_sample, fake_sample, si_sample: (calls.append(("D", trainer.module.global_step)), au_ret)[1]
    gt.au_eval_step = lambda trainer, real_sample, fake_sample, si_sample: (calls.append(("Deval", trainer.module.global_step)), au_ret)[1]
    try:
        class DS(torch.utils.data.Dataset):
            def __len__(self):
                return 12

            def __getitem__(self, i):
                return {"real_sample": torch.zeros(3, 1, 4, 4), "leaked_sample": torch.zeros(1, 1, 4, 4), "si_sample": torch.zeros(2, 1, 4, 4), "class": i}
        tr = Wrap(StubTrainer())
        logger = G.Logger(log_dir=str(tmp_path / "logs"), img_dir=str(tmp_path / "imgs"))
        gt.train_epoch(device=torch.device("cpu"), logger=logger, epoch=0, trainer=tr, train_ds=DS(), val_ds=DS(), train_batch_size=2,
                       val_batch_size=4, num_workers=0, save_every=4, eval_every=5, save_imgs_every=10 ** 9, train_eval_indices=[],
                       val_eval_indices=[], tb_log_every=2, tb_log_enc_every=10 ** 9, n_au_steps=2)
    finally:
        gt.gim_step, gt.im_eval_step, gt.au_train_step, gt.au_eval_step = orig
        gt.mb.custom_std = orig_std
    assert [c[1] for c in calls if c[0] == "G+D"] == [1, 3, 5]          # (global_step + 1) % n_au_steps == 0 trains G
    assert [c[1] for c in calls if c[0] == "D"] == [0, 2, 4]            # the D step runs every iteration (inside G+D otherwise)
    assert tr.module.saved == [(0, 0), (0, 4)]
    assert sum(1 for c in calls if c[0] == "Deval") == 3 * 2            # eval at steps 0 and 5: 12 // 4 = 3 batches each
    assert [s_ for s_, _ in logger.stats["train_losses"]["dis_loss"]] == [0, 2, 4]
    assert logger.get_last_scalar("eval accuracy", "dis acc") == 1.0 and logger.get_last_scalar("nope", "x", default=7.0) == 7.0
    logger.save_stats("stats.p")
    l2 = G.Logger(log_dir=str(tmp_path / "logs"), img_dir=str(tmp_path / "imgs"))
    l2.load_stats("stats.p")
    assert l2.stats == logger.stats
    logger.add_imgs(torch.rand(7, 3, 4, 4), "cat a", "k", 3)
    assert len(os.listdir(str(tmp_path / "imgs" / "cat_a" / "k"))) == 1


def test_roc_auc_matches_sklearn():
    """authentication_eval.roc_auc (rank statistic with mid-ranks) == sklearn.metrics.roc_auc_score, ties included."""
    import numpy as np
    from sklearn.metrics import roc_auc_score
    from optimalstrategiesagainstgenerativeattacks_amd.authentication_eval import comp_acc, roc_auc
    rng = np.random.default_rng(0)
    for trial in range(5):
        y = rng.integers(0, 2, 200)
        s = np.round(rng.normal(size=200) + 0.7 * y, 1 if trial % 2 else 6)   # coarse rounding -> ties
        assert abs(roc_auc(y, s) - roc_auc_score(y, s)) < 1e-12
    acc, acc_f, acc_r = comp_acc(torch.tensor([1, 1, 0, 1]), torch.tensor([0, 1, 0, 0]))
    assert float(acc_r) == 0.75 and float(acc_f) == 0.75 and float(acc) == 0.75


# ---------------------------------------------------------------------------------------------------
# bench.py --gpus N launches itself; the library keeps no process-wide state
# ---------------------------------------------------------------------------------------------------
def test_bench_self_launch_dry_run_gloo_world2():
    """`python bench.py --gpus 2` with no launcher around it (WORLD_SIZE unset) starts two ranks of itself, which rendezvous
    (gloo here, RCCL on the GPU node), all-reduce once, and rank 0's ONE JSON line comes out of the parent; the parent's return
    code is the worst rank's.  --dry-run stops before anything touches a GPU."""
    import json
    import subprocess
    env = {k_: v for k_, v in os.environ.items() if k_ not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["GIM_BENCH_BACKEND"] = "gloo"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--dry-run"],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["dry_run"] and line["n_gpus"] == 2 and line["rccl_ranks"] == 2 and line["backend"] == "gloo"
    assert line["steps"] == 3 and line["warmup"] == 1 and line["config"]["global_batch"] == 32
    # a launcher's environment is used as given: WORLD_SIZE that disagrees with --gpus is refused, and the failure propagates
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run"],
                         env=dict(env, WORLD_SIZE="1", RANK="0"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert bad.returncode != 0 and "WORLD_SIZE=1 but --gpus 2" in bad.stderr


def test_bench_dump_outputs_names_dtype_and_budget(tmp_path):
    """bench.dump_outputs: one float32 .npy per returned tensor, named after gim_step's tuples; an output larger than its share
    of the byte budget is replaced by the same seeded sample of its elements on every call.  (A child process: importing
    bench sets GPU_MAX_HW_QUEUES in its environment.)"""
    import subprocess
    import numpy as np
    code = (
        "import sys, torch; sys.path.insert(0, %r); import bench\n"
        "bench.DUMP_BUDGET_BYTES = 1 << 16\n"
        "g = torch.Generator().manual_seed(0)\n"
        "big = torch.rand(4, 5, 3, 32, 32, generator=g, dtype=torch.float64)\n"
        "im = (torch.tensor(1.5), big, torch.rand(4, 5, generator=g))\n"
        "au = tuple(torch.tensor(float(i)) for i in range(6)) + (torch.rand(4, 5) > 0.5, torch.rand(4, 5) > 0.5, torch.rand(4, 5))\n"
        "bench.dump_outputs((im, au), sys.argv[1]); bench.dump_outputs((im, au), sys.argv[2])\n"
        "torch.save(big, sys.argv[3])\n" % ROOT)
    a, b, big = str(tmp_path / "a"), str(tmp_path / "b"), str(tmp_path / "big.pt")
    r = subprocess.run([sys.executable, "-c", code, a, b, big], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    files = sorted(os.listdir(a))
    assert files == sorted(n_ + ".npy" for n_ in ("g_loss", "g_fake_sample", "g_au_out", "d_loss", "d_loss_on_real", "d_loss_on_fake",
                                                   "d_reg", "d_out_on_real", "d_out_on_fake", "d_pred_on_real", "d_pred_on_fake",
                                                   "d_fake_out")), files
    total = 0
    for f in files:
        x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        assert x.dtype == np.float32 and np.array_equal(x, y), f
        total += x.nbytes
    assert total <= 1 << 16
    assert np.load(os.path.join(a, "g_loss.npy")).shape == () and float(np.load(os.path.join(a, "g_loss.npy"))) == 1.5 and np.load(os.path.join(a, "g_au_out.npy")).shape == (4, 5)
    s = np.load(os.path.join(a, "g_fake_sample.npy"))
    full = torch.load(big).numpy().astype(np.float32).reshape(-1)
    assert s.ndim == 1 and 0 < s.size < full.size and np.isin(s, full).all()     # a sample of the real elements, not a summary


def test_conv_shape_struct_matches_the_header():
    """The ctypes mirror of gim_conv_shape has the header's fields in the header's order (matrix path and launch overrides are
    per-call fields: the library has no precision / tuning globals) - and so has the mirror of every other struct of the header
    (the job tables of the grouped launches), each field at the offset the header's field sizes give it."""
    from optimalstrategiesagainstgenerativeattacks_amd import _lib
    header = open(os.path.join(ROOT, "include", "gim_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} gim_conv_shape;", header).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += [f.strip() for f in decl.split(None, 1)[1].split(",")]
    assert fields == [f for f, _ in _lib.GimConvShape._fields_], fields
    assert ctypes.sizeof(_lib.GimConvShape) == 4 * len(fields)
    assert "gim_conv_precision" not in header and "gim_conv_tune_override" not in header

    structs = re.findall(r"typedef struct \{([^}]*)\} (gim_\w+);", header)
    assert len(structs) == header.count("typedef struct") >= 6
    sizes = {}
    for body, name in structs:
        mirror = getattr(_lib, "".join(part.capitalize() for part in name.split("_")))      # gim_sn_job -> GimSnJob: must exist
        expect, off = [], 0
        for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";"):
            decl = decl.strip()
            if not decl:
                continue
            if "*" in decl:      # "const float* w"
                size, names = 8, [decl.rsplit("*", 1)[1]]
            else:                # "int32_t Cout, Cin, KH, reserved"
                ctype, names = decl.split(None, 1)
                size, names = {"int64_t": 8, "int32_t": 4, "float": 4}[ctype], names.split(",")
            for f in names:
                expect.append((f.strip(), off))
                off += size
        assert [(f, getattr(mirror, f).offset) for f, _ in mirror._fields_] == expect, name
        assert ctypes.sizeof(mirror) == off, name
        sizes[name] = off
    assert sizes == {"gim_conv_shape": 68, "gim_infer_conv": 28, "gim_fold_job": 32, "gim_sn_job": 72, "gim_wgrad_job": 104,
                     "gim_gemm_job": 88}


def test_job_table_layout():
    """ops.layout_tables: the job structs and the int32 tables of a grouped launch as one buffer of 16-byte-aligned sections; an
    empty table is a placeholder row of zeros."""
    import struct
    from optimalstrategiesagainstgenerativeattacks_amd import _lib, ops
    jobs = (_lib.GimFoldJob * 3)((0x7f0000001000, 0x7f0000002000, 3, 5, 1, 0), (0x7f0000003000, 0x7f0000004000, 16, 8, 3, 0),
                                 (0x7f0000005000, 0x7f0000006000, 72, 64, 3, 0))
    tab = [(0, 0), (1, 0), (2, 1)]
    blob, offsets = ops.layout_tables(jobs, tab, [])
    sections = [bytes(jobs), struct.pack("<6i", 0, 0, 1, 0, 2, 1), bytes(8)]
    assert len(sections[0]) == 3 * 32 and len(offsets) == 3 and offsets[0] == 0
    for off, sec in zip(offsets, sections):
        assert off % 16 == 0 and blob[off:off + len(sec)] == sec
    assert offsets == sorted(offsets) and all(b >= a + len(sec) for a, b, sec in zip(offsets, offsets[1:], sections))
    assert len(blob) == offsets[-1] + len(sections[-1])
    # a table whose length is no multiple of 16 bytes pushes the next section to the next boundary
    blob, offsets = ops.layout_tables(jobs, [(7, 8, 9)], [(1, 2)])
    assert offsets == [0, 96, 112] and blob[96:108] == struct.pack("<3i", 7, 8, 9) and blob[112:] == struct.pack("<2i", 1, 2)


def test_job_table_cache_is_lru():
    """ops._TableCache: build runs once per miss, a hit renews the entry, the least recently used one leaves beyond the capacity."""
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    built = []

    def build_for(sig):
        def build():
            built.append(sig)
            return ("table", sig)
        return build
    cache = ops._TableCache("test", 2)
    assert len(cache) == 0
    assert cache.get("a", build_for("a")) == ("table", "a") and cache.get("b", build_for("b")) == ("table", "b")
    assert len(cache) == 2 and built == ["a", "b"]
    assert cache.get("c", build_for("c")) == ("table", "c")
    assert len(cache) == 2 and list(cache) == ["b", "c"]                 # the first signature was evicted
    assert cache.get("b", build_for("b")) == ("table", "b") and built == ["a", "b", "c"]
    assert list(cache) == ["c", "b"]                                     # the hit moved its entry to the end ...
    cache.get("d", build_for("d"))
    assert list(cache) == ["b", "d"] and built == ["a", "b", "c", "d"]   # ... so the other one left
    cache.get("a", build_for("a"))
    assert built == ["a", "b", "c", "d", "a"] and len(cache) == 2
    cache.clear()
    assert len(cache) == 0
    unbounded = ops._TableCache("test")
    for i in range(100):
        unbounded.get(i, build_for(i))
    assert len(unbounded) == 100


def test_library_sources_read_no_environment_and_keep_no_mutable_globals():
    """include/gim_hip.h promises: no environment variables, no mutable process-wide state.  Checked on the sources: no getenv,
    every namespace-scope `static` object is const / constexpr, and the only thread_local is the error string's definition."""
    csrc = os.path.join(ROOT, "optimalstrategiesagainstgenerativeattacks_amd", "csrc")
    for f in sorted(os.listdir(csrc)):
        if not f.endswith((".hip", ".h")):
            continue
        src = open(os.path.join(csrc, f)).read()
        assert "getenv" not in src, f
        assert "GIM_DBG" not in src, f
        for mt in re.finditer(r"^static\s+(?!inline|const|constexpr|thread_local|__device__|__global__|void|int\s+\w+\(|bool\s+\w+\(|Geo\s+\w+\(|"
                              r"WgPlan\s+\w+\(|IgemmPlan\s+\w+\(|size_t\s+\w+\(|float\s+\w+\(|long\s+long\s+\w+\()([^;{(]*)[;=]", src, re.M):
            raise AssertionError("%s: mutable file-scope static: %s" % (f, mt.group(0)))
        tls = [ln.strip() for ln in src.splitlines() if "thread_local" in ln]
        assert tls == (['static thread_local char g_err[512] = "";'] if f == "adam.hip" else []), (f, tls)


def test_episode_sampler_ranks_stay_in_step_over_epochs():
    """Data-parallel episode sharding (training/gim_img_training.py:406-411 scatters the batch over devices): every rank's
    process shuffles the SAME epoch order - also in later epochs, although each rank has drawn a different, data-dependent
    number of random values for its own episodes in between (classes of unequal size) - and the rank slices of a global batch
    are disjoint and complete."""
    from optimalstrategiesagainstgenerativeattacks_amd.data import EpisodeSampler
    sizes = [9, 30, 8, 17, 12, 25, 8, 40]
    offs = [0]
    for s_ in sizes:
        offs.append(offs[-1] + s_)
    world, bs = 2, 4
    ranks = [EpisodeSampler(offs, 1, 3, 4, example_cnt_per_class=2, mirror=True, seed=7) for _ in range(world)]   # one per process
    single = EpisodeSampler(offs, 1, 3, 4, example_cnt_per_class=2, mirror=True, seed=7)
    for epoch in range(4):
        per_rank = [list(r.epoch_rows(bs, True, True, rank, world)) for rank, r in enumerate(ranks)]
        whole = list(single.epoch_rows(bs, True, True, 0, 1))
        assert len(per_rank[0]) == len(per_rank[1]) == len(whole) == len(single) // bs
        for i, rows in enumerate(whole):
            assert per_rank[0][i] + per_rank[1][i] == rows, (epoch, i)     # the two slices ARE the global batch, in order
        for rank, r in enumerate(ranks):                                     # each rank now draws its episodes (different counts)
            for rows in per_rank[rank]:
                idx, flip = r.draw(rows, rank)
                assert idx.shape == (len(rows), 8) and all(len(set(row.tolist())) == 8 for row in idx)
        single.draw(whole[0], 0)
    a, _ = ranks[0].draw([1, 1], 0)
    b, _ = ranks[1].draw([1, 1], 1)
    assert not (a == b).all()      # ranks draw different images


def test_deterministic_switch_forces_one_k_slice_and_slab_weight_gradients():
    """ops.set_deterministic (GIM_DETERMINISTIC=1): every convolution shape carries tune_ksplit = 1, and the library then plans
    ONE K slice (no float atomics) for a forward / dgrad launch that splits K by default; the weight-gradient path asks for slabs.
    (Bit-reproducibility itself is a GPU test: tests/test_gpu_models.py::test_deterministic_mode_is_bit_reproducible.)"""
    from optimalstrategiesagainstgenerativeattacks_amd import _lib, ops
    lib = _lib.load()

    def plan(sh, kind):
        out = (ctypes.c_int32 * 8)()
        assert lib.gim_conv_launch_plan(ctypes.byref(sh), kind, ctypes.cast(out, ctypes.c_void_p)) == 0
        return list(out)
    prev = ops.set_deterministic(False)
    try:
        args = (80, 4, 4, 512, 512, 3, 0, 0.2)      # 80 images of 4 x 4 pixels: 1280 output pixels, K = 4608 - splits K by default
        sh = ops._shape(*args)
        assert sh.tune_ksplit == 0 and plan(sh, 0)[3] > 1 and plan(sh, 1)[3] > 1
        assert ops.set_deterministic(True) is False and ops.deterministic()
        sh = ops._shape(*args)
        assert sh.tune_ksplit == 1 and plan(sh, 0)[3] == 1 and plan(sh, 1)[3] == 1
        assert plan(sh, 0)[7] & 255 == 0      # and the tap-major loop (one K order whatever the batch): not the patch-resident kernel
        # ... on position-major rows (a map of <= 16 pixels, >= 32 images): plan[7] >> 8 = the skipped share of its K steps in 1/1000.
        # 80 images on a 4 x 4 map in 64-row tiles: between nothing and the 30.6 % of (pixel, tap) pairs that fall into the padding
        assert 150 <= plan(sh, 0)[7] >> 8 <= 306 and 150 <= plan(sh, 1)[7] >> 8 <= 306, (plan(sh, 0), plan(sh, 1))
        one = ops._shape(64, 2, 2, 512, 512, 3, 0, 0.2)   # 64 images, 2 x 2 map: one tile = one pixel, 4 of its 9 taps are inside the map
        assert plan(one, 0)[7] >> 8 == 556 and plan(one, 1)[7] >> 8 == 556, (plan(one, 0), plan(one, 1))
        few = ops._shape(16, 4, 4, 512, 512, 3, 0, 0.2)   # 16 images: image-major rows, nothing skipped
        big = ops._shape(80, 16, 16, 128, 128, 3, 0, 0.2)
        assert plan(few, 0)[7] >> 8 == 0 and plan(big, 0)[7] >> 8 == 0
        assert lib.gim_conv2d_wgrad_slabs(ctypes.byref(sh)) >= 1
    finally:
        ops.set_deterministic(prev)
    assert ops.deterministic() == prev


def _pin_worker(rank, world, q):
    from optimalstrategiesagainstgenerativeattacks_amd.training_utils import pin_rank_to_cores
    before = sorted(os.sched_getaffinity(0))
    got = pin_rank_to_cores(rank, world)
    q.put((rank, before, got, sorted(os.sched_getaffinity(0))))


@pytest.mark.skipif(not hasattr(os, "sched_setaffinity") or len(os.sched_getaffinity(0)) < 4, reason="needs >= 4 cores to split")
def test_ranks_pin_themselves_to_disjoint_core_sets():
    """pin_rank_to_cores: the cores this job may use are dealt out in contiguous, disjoint blocks by LOCAL_RANK (bench.py and
    train_gim_imgs call it before the first GPU call); one rank alone changes nothing."""
    from optimalstrategiesagainstgenerativeattacks_amd.training_utils import pin_rank_to_cores
    assert pin_rank_to_cores(0, 1) is None
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_pin_worker, args=(r, 2, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (_, before0, got0, after0), (_, before1, got1, after1) = res
    assert before0 == before1 and got0 == after0 and got1 == after1
    assert not set(got0) & set(got1) and len(got0) == len(got1) == len(before0) // 2
    assert set(got0) | set(got1) <= set(before0)


def test_hw_queue_default_is_reported():
    """Importing the package before the first GPU call sets GPU_MAX_HW_QUEUES=8 unless the user chose a value; hw_queues_state()
    says which value is in force and whether HIP had already been initialised (then the default could not take effect and the
    import warns) - ADVICE r03; bench.py prints it with the result of the start-up spin test of the engine's streams."""
    import subprocess
    code = ("import os, json, warnings\n"
            "os.environ.pop('GPU_MAX_HW_QUEUES', None)\n"
            "import optimalstrategiesagainstgenerativeattacks_amd as G\n"
            "print(json.dumps(G.hw_queues_state()))\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300,
                       env={k: v for k, v in os.environ.items() if k != "GPU_MAX_HW_QUEUES"})
    assert r.returncode == 0, r.stderr[-2000:]
    import json
    st = json.loads(r.stdout.strip().splitlines()[-1])
    assert st == {"GPU_MAX_HW_QUEUES": "8", "preset_by_user": False, "hip_initialised_before_import": False}
    r = subprocess.run([sys.executable, "-c", code.replace("os.environ.pop('GPU_MAX_HW_QUEUES', None)", "os.environ['GPU_MAX_HW_QUEUES'] = '4'")],
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    st = json.loads(r.stdout.strip().splitlines()[-1])
    assert st["GPU_MAX_HW_QUEUES"] == "4" and st["preset_by_user"]


def test_gaussian_loop_scatters_one_global_batch_over_the_ranks(monkeypatch):
    """train() of the Gaussian game under EpisodeParallel: every rank draws the SAME global batch (identical host
    seeds) and trains on ITS slice - nn.DataParallel scatters one batch of batch_size (training/gim_gaussian_training.py:198-201) -
    instead of every rank training on the whole batch.  The step itself is stubbed (it needs the GPU); what is checked is what the
    step is handed, for world_size 2 against world_size 1."""
    from optimalstrategiesagainstgenerativeattacks_amd import gim_gaussian_training as gg
    from optimalstrategiesagainstgenerativeattacks_amd.training_utils import EpisodeParallel
    seen = []

    def fake_step(trainer, leaked, real, si, z=None):
        seen.append((leaked.clone(), real.clone(), si.clone(), None if z is None else z.clone()))
        B = leaked.size(0)
        s0 = torch.zeros(())
        return (s0, real, s0), (s0, s0, s0, s0, s0, s0, torch.ones(B, 1, dtype=torch.bool), torch.zeros(B, 1, dtype=torch.bool), real)
    monkeypatch.setattr(gg, "gim_step", fake_step)

    class Mod:
        m, n, k = 1, 3, 4
        gs = 0      # the first iteration is global step 1: no statistics / checkpoint cadence hit (those run GPU kernels)

        def do_global_step(self):
            self.gs += 1

        def get_global_step(self):
            return self.gs

        def save(self):
            pass

    class Log:
        def add_scalar(self, **kw):
            pass
    runs = {}
    for world, rank in ((1, 0), (2, 0), (2, 1)):
        tr = EpisodeParallel(Mod())
        tr.world_size, tr.rank = world, rank
        torch.manual_seed(11)
        del seen[:]
        gg.train(torch.device("cpu"), tr, Log(), n_iters=2, batch_size=6, src_dim=5, src_sigma=1.0, prior_sigma=2.0,
                 save_stats_every=1000, save_every=1000, host_noise=True)
        runs[(world, rank)] = list(seen)
    for it in range(2):
        whole = runs[(1, 0)][it]
        for j in range(4):
            assert whole[j].shape[0] == 6
            both = torch.cat([runs[(2, 0)][it][j], runs[(2, 1)][it][j]])
            assert torch.equal(both, whole[j]), (it, j)


def test_training_step_runs_autograd_nodes_on_the_calling_thread():
    """ops.caller_thread_backward(): the context the training step's .backward() / autograd.grad() calls run under switches torch's
    autograd engine to the calling thread (every node of the engine is a Python Function: the hand-off to the per-device worker thread
    cost 15-25 % of the host's time per step, profiles/r04_m_host_enqueue.txt) and restores the previous mode on exit."""
    import torch
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    assert ops._CALLER_THREAD_BACKWARD      # the default (GIM_MT_AUTOGRAD unset)
    before = torch.autograd.is_multithreading_enabled()
    with ops.caller_thread_backward():
        assert not torch.autograd.is_multithreading_enabled()
        x = torch.ones(3, requires_grad=True)
        (x * 2).sum().backward()
        assert torch.equal(x.grad, torch.full((3,), 2.0))
    assert torch.autograd.is_multithreading_enabled() == before


def test_model_train_eval_switch_every_submodule():
    """GIMFaceImpersonator / GIMFaceAuthenticator override train() with a direct walk (gim_img_models._set_training: the reference calls
    .train() on both networks every step): same contract as nn.Module.train - every submodule switched, eval() = train(False), a
    non-boolean mode refused, self returned."""
    import optimalstrategiesagainstgenerativeattacks_amd as G
    for net in (G.get_im(16, 1, 32), G.get_au(16, 1, 32)):
        assert net.eval() is net and not any(m.training for m in net.modules())
        assert net.train() is net and all(m.training for m in net.modules())
        net.train(False)
        assert not any(m.training for m in net.modules())
        with pytest.raises(ValueError):
            net.train("yes")


# The conv calls of the benchmark networks (vox64 at 16 episodes, om32 at 32) and their neighbours just across each predicate.
#  name, (N, H, W, Cin, Cout, KH, ups, pre_slope, pool, res_ups, has_res, linear),
#  expected: fwd (tune_tile 0), fwd (tune_tile -1), dgrad, dgrad without the parameter, dgrad + res_half, dgrad fp16, dgrad fp16 + res_half,
#            wgrad into .grad, wgrad with an untargeted bias, wgrad without a target, wgrad without target and spectral norm
_X4, _X2, _T, _P, _U, _R = ("xfold", 4), ("xfold", 2), ("t", 0), ("plain", 0), ("ups", 0), ("res", 0)
_Q, _QR, _S, _D = ("queued", 1), ("queued_rows", 1), ("slabs", 1), ("direct", 1)
_ROUTE_ROWS = [
    ("img 9x9 3->64", (240, 64, 64, 3, 64, 9, 0, 1.0, False, False, False, False),             ("rows", "plain", _X4, _P, _X4 + (True,), _X4, _X4 + (True,), _QR, _S, _S, _D)),
    ("img 9x9 6->64", (80, 64, 64, 6, 64, 9, 0, 1.0, False, False, False, False),              ("rows", "plain", _X4, _P, _X4 + (True,), _X4, _X4 + (True,), _QR, _S, _S, _D)),
    ("img 9x9 1->64 (om32)", (480, 32, 32, 1, 64, 9, 0, 1.0, False, False, False, False),      ("rows", "plain", _X4, _P, _X4 + (True,), _X4, _X4 + (True,), _QR, _S, _S, _D)),
    ("img 9x9 2->64 (om32)", (160, 32, 32, 2, 64, 9, 0, 1.0, False, False, False, False),      ("rows", "plain", _X4, _P, _X4 + (True,), _X4, _X4 + (True,), _QR, _S, _S, _D)),
    ("img 9x9 8->64", (16, 64, 64, 8, 64, 9, 0, 1.0, False, False, False, False),              ("plain", "plain", _X2, _P, _X2 + (True,), _X2, _X2 + (True,), _Q, _S, _S, _D)),
    ("img 3x3 7->64 lrelu", (16, 64, 64, 7, 64, 3, 0, 0.2, False, False, False, False),        ("rows", "plain", _X2, _P, _X2 + (True,), _X2, _X2 + (True,), _QR, _S, _S, _D)),
    ("img 3x3 3->64 W=2 lrelu", (16, 2, 2, 3, 64, 3, 0, 0.2, False, False, False, False),      ("rows", "plain", _T, _P, _T + (True,), _T, _T + (True,), _QR, _S, _S, _D)),
    ("img 3x3 3->3", (16, 64, 64, 3, 3, 3, 0, 1.0, False, False, False, False),                ("plain", "plain", _P, _P, _P + (True,), _P, _P + (True,), _Q, _S, _S, _D)),
    ("img 1x1 3->64", (240, 64, 64, 3, 64, 1, 0, 1.0, False, False, False, False),             ("plain", "plain", _T, _P, _T + (True,), _T, _T + (True,), _Q, _S, _S, _D)),
    ("out 9x9 64->3 ups", (80, 64, 64, 64, 3, 9, 1, 0.2, False, False, False, False),          ("subpixel", "plain", _P, _P, _P + (True,), _P, _P + (True,), _Q, _S, _S, _S)),
    ("out 9x9 64->1 ups (om32)", (160, 32, 32, 64, 1, 9, 1, 0.2, False, False, False, False),  ("subpixel", "plain", _P, _P, _P + (True,), _P, _P + (True,), _Q, _S, _S, _S)),
    ("out 9x9 64->3 ups + res", (80, 64, 64, 64, 3, 9, 1, 0.2, False, False, True, False),     ("plain", "plain", _P, _P, _P + (True,), _P, _P + (True,), _Q, _S, _S, _S)),
    ("out 7x7 64->3 ups", (80, 64, 64, 64, 3, 7, 1, 0.2, False, False, False, False),          ("plain", "plain", _P, _P, _P + (True,), _P, _P + (True,), _Q, _S, _S, _S)),
    ("pool 3x3 64->128 + res", (240, 64, 64, 64, 128, 3, 0, 0.2, True, False, True, False),    ("plain", "plain", _P, _P, _P + (True,), _T, _T + (True,), _Q, _S, _S, _S)),
    ("subpixel 3x3 512->256", (80, 16, 16, 512, 256, 3, 1, 0.2, False, False, False, False),   ("plain", "plain", _P, _P, _P + (True,), _T, _T + (True,), _Q, _S, _S, _S)),
    ("ups 1x1 512->256", (80, 16, 16, 512, 256, 1, 1, 1.0, False, False, False, False),        ("plain", "plain", _U, _U, _U + (True,), _U, _U + (True,), _Q, _S, _S, _D)),
    ("skip 1x1 64->128", (240, 32, 32, 64, 128, 1, 0, 1.0, False, False, False, False),        ("plain", "plain", _P, _P, _P + (True,), _T, _T + (True,), _Q, _S, _S, _D)),
    ("plain 3x3 64->64 lrelu", (240, 64, 64, 64, 64, 3, 0, 0.2, False, False, False, False),   ("plain", "plain", _P, _P, _R + (False,), _T, _T + (True,), _Q, _S, _S, _D)),
    ("plain 3x3 128->128", (240, 32, 32, 128, 128, 3, 0, 1.0, False, False, False, False),     ("plain", "plain", _P, _P, _P + (True,), _T, _T + (True,), _Q, _S, _S, _D)),
    ("res_ups 3x3 256->256", (80, 32, 32, 256, 256, 3, 0, 0.2, False, True, True, False),      ("plain", "plain", _P, _P, _R + (False,), _T, _T + (True,), _Q, _S, _S, _D)),
    ("small map 3x3 512->512", (240, 4, 4, 512, 512, 3, 0, 0.2, False, False, False, False),   ("plain", "plain", _P, _P, _R + (False,), _T, _T + (True,), _Q, _S, _S, _D)),
    ("plain 3x3 64->40 lrelu", (16, 16, 16, 64, 40, 3, 0, 0.2, False, False, False, False),    ("plain", "plain", _P, _P, _R + (False,), _P, _R + (False,), _Q, _S, _S, _D)),
    ("linear 512->512", (16, 1, 1, 512, 512, 1, 0, 1.0, False, False, False, True),            ("plain", "plain", _P, _P, _P + (True,), _T, _T + (True,), _Q, _S, _S, _D)),
    ("linear 8192->512 lrelu", (16, 1, 1, 8192, 512, 1, 0, 0.2, False, False, False, True),    ("plain", "plain", _P, _P, _R + (False,), _T, _T + (True,), _Q, _S, _S, _D)),
]
# gim_conv2d_wgrad_slabs of each row's shape (the library's answer on the parent commit; it is the same in deterministic mode)
_ROUTE_SLABS = [512, 512, 960, 320, 128, 512, 1, 512, 1024, 205, 320, 205, 160, 128, 8, 40, 480, 205, 114, 29, 8, 32, 1, 1]


def _route_table(ops):
    out = []
    for name, (N, H, W, Cin, Cout, KH, ups, slope, pool, res_ups, has_res, linear), _ in _ROUTE_ROWS:
        g = ops.ConvGeom.make(N, H, W, Cin, Cout, KH, ups, slope, pool, res_ups, has_res=has_res, linear=linear)
        assert g.key == (N, H, W, Cin, Cout, KH, ups, int(pool), g.fold) and g.fold == int(bool(pool or (ups and KH > 1))), name
        sh = g.shape("wgrad")
        rows_copy = ops._fwd_route(g, 0) == "rows"      # the padded copy exists where the forward made it
        dg = [ops._dgrad_route(g, 0, True), ops._dgrad_route(g, 0, False), ops._dgrad_route(g, 0, True, True),
              ops._dgrad_route(g, 1, True), ops._dgrad_route(g, 1, True, True)]
        out.append((ops._fwd_route(g, 0), ops._fwd_route(g, -1), dg[0][:2], dg[1][:2], dg[2], dg[3][:2], dg[4],
                    ops._wgrad_route(g, sh, True, True, False, rows_copy), ops._wgrad_route(g, sh, True, True, True, rows_copy),
                    ops._wgrad_route(g, sh, False, True), ops._wgrad_route(g, sh, False, False)))
        assert not (dg[0][2] or dg[1][2] or dg[3][2]), name      # nothing to add without a res_half
    return out


def test_conv_routes_are_the_parent_commits_inline_dispatch():
    """ops._fwd_route / _dgrad_route / _wgrad_route on the conv calls of the benchmark networks.  The expected tags are literals:
    they were obtained by evaluating the inline conditions of ConvFn.forward, _conv_dgrad and _conv_wgrad of the commit before the
    route functions existed on these rows (not by running the functions under test).  Then every A/B switch, deterministic mode and
    the queue switch: each moves exactly the routes it names - the expectations under a switch are the same literals with that one
    substitution, which is what the parent's conditions gave, row by row."""
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    assert not ops.deterministic() and ops.matrix_path() == "fp32" and ops.wgrad_queue.enabled and not ops._WGRAD_SLABS
    assert ops._ROWS_FORM and ops._MERGED_SUBPIXEL and ops._NARROW_DGRAD_T and ops._NARROW_XFOLD
    base = [e for _, _, e in _ROUTE_ROWS]
    got = _route_table(ops)
    for (name, _, want), have in zip(_ROUTE_ROWS, got):
        assert have == want, (name, have, want)

    def flipped(setter, restore, expect):
        setter()
        try:
            have = _route_table(ops)
        finally:
            restore()
        want = [expect(i, e) for i, e in enumerate(base)]
        for (name, _, _), h, w_ in zip(_ROUTE_ROWS, have, want):
            assert h == w_, (name, h, w_)
        assert have != base      # the switch does move something on this table
        assert _route_table(ops) == base

    def module_switch(name, value, expect):
        old = getattr(ops, name)
        flipped(lambda: setattr(ops, name, value), lambda: setattr(ops, name, old), expect)

    def sub(e, cols, fn):
        return tuple(fn(v) if c in cols else v for c, v in enumerate(e))
    FWD, DGRAD, WGRAD = (0, 1), (2, 3, 4, 5, 6), (7, 8, 9, 10)
    # the row-contiguous forward, and with it the padded copy the queued weight gradient reads
    module_switch("_ROWS_FORM", False, lambda i, e: sub(sub(e, FWD, lambda v: "plain" if v == "rows" else v), WGRAD, lambda v: _Q if v == _QR else v))
    module_switch("_MERGED_SUBPIXEL", False, lambda i, e: sub(e, FWD, lambda v: "plain" if v == "subpixel" else v))
    module_switch("_NARROW_XFOLD", False, lambda i, e: sub(e, DGRAD, lambda v: _T + v[2:] if v[0] == "xfold" else v))
    # the k-contiguous dgrad of the image layers (rows 0-6 and 8: <= 8 input channels, 64 output channels) goes back to the plain
    # kernel - with a res_half, to its fused form where there is a LeakyReLU mask (rows 5, 6); the fp16 path's own "t" stays
    narrow = {0, 1, 2, 3, 4, 5, 6, 8}
    module_switch("_NARROW_DGRAD_T", False, lambda i, e: e if i not in narrow else sub(sub(e, (2, 5), lambda v: _P), (4, 6), lambda v: _R + (False,) if i in (5, 6) else _P + (True,)))

    def slabbed(i, e, also_queued):      # the non-queued forms ask the library for the slab count; one launch stays "direct" only for 1 slab
        ns = _ROUTE_SLABS[i]
        e = sub(e, (8, 9) + ((7,) if also_queued else ()), lambda v: ("slabs", ns))
        return sub(e, (10,), lambda v: v if (v == _D and ns == 1) else ("slabs", ns))
    module_switch("_WGRAD_SLABS", True, lambda i, e: slabbed(i, e, False))
    flipped(lambda: ops.set_deterministic(True), lambda: ops.set_deterministic(False), lambda i, e: slabbed(i, e, True))
    flipped(lambda: setattr(ops.wgrad_queue, "enabled", False), lambda: setattr(ops.wgrad_queue, "enabled", True), lambda i, e: sub(e, (7,), lambda v: _S))


def test_conv_geom_derived_values_and_activated_storage():
    """ops.ConvGeom: the derived sizes of the pool / sub-pixel folds and of a linear, the record ConvDgradFn differentiates, the shape
    struct per launch kind with its _TUNE_OVERRIDE entry, and the one activated-storage decision (not for a split-K launch)."""
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    pool = ops.ConvGeom.make(240, 64, 64, 64, 128, 3, 0, 0.2, True, has_bias=True, has_res=True)
    assert (pool.fold, pool.out_shape, pool.out_pixels, pool.K, pool.KFF) == (1, (240, 32, 32, 128), 240 * 32 * 32, 576, 1024)
    assert pool.key == (240, 64, 64, 64, 128, 3, 0, 1, 1)
    lin = pool.linear_map()
    assert (lin.pre_slope, lin.has_bias, lin.has_res, lin.res_ups, lin.x_act, lin.pool, lin.fold, lin.key) == (1.0, False, False, False, False, True, 1, pool.key)
    fc = ops.ConvGeom.make(16, 1, 1, 512, 10, 1, linear=True)
    assert (fc.fold, fc.out_shape, fc.out_pixels, fc.K, fc.KFF) == (0, (16, 10), 16, 512, 512)
    sh = pool.shape("wgrad", 1.0)
    assert (sh.N, sh.H, sh.Cin, sh.Cout, sh.KH, sh.pool, sh.wfold, sh.res_ups, sh.pre_slope, sh.tune_tile) == (240, 64, 64, 128, 3, 1, 1, 0, 1.0, 0)
    assert abs(pool.shape("dgrad").pre_slope - 0.2) < 1e-7
    ops._TUNE_OVERRIDE[("dgrad", pool.key)] = (7, 3)
    try:
        assert (pool.shape("dgrad").tune_tile, pool.shape("dgrad").tune_ksplit) == (7, 3)
        assert pool.shape("fwd").tune_tile == 0 and pool.shape(None).tune_tile == 0
    finally:
        ops._TUNE_OVERRIDE.clear()
    split = ops.ConvGeom.make(80, 4, 4, 512, 512, 3, 0, 0.2)        # splits K (test_deterministic_switch_...): stores raw y
    whole = ops.ConvGeom.make(240, 64, 64, 64, 64, 3, 0, 0.2)
    last = ops.ConvGeom.make(80, 64, 64, 64, 3, 9, 1, 0.2)           # stacked sub-pixel form: activates in its depth-to-space copy
    assert ops._launch_plan(split.shape("fwd"), 0, split.key).ksplit > 1 and ops._launch_plan(whole.shape("fwd"), 0, whole.key).ksplit == 1
    assert [ops._stores_activated(g, 0.2) for g in (split, whole, last, fc)] == [False, True, True, False]
    assert not ops._stores_activated(whole, 1.0)
    n = len(ops._SPLITS_K)
    assert n >= 2 and ops._launch_plan(whole.shape("fwd"), 0, whole.key) is ops._launch_plan(whole.shape("fwd"), 0, whole.key) and len(ops._SPLITS_K) == n
    prev = ops.set_deterministic(not ops.deterministic())           # the cached plans were made for the other mode
    try:
        assert not ops._SPLITS_K
    finally:
        ops.set_deterministic(prev)


def test_rect_cases_reach_the_kernel_families_they_name():
    """tests/helpers.py RECT_CASES (the GPU parity cases on maps with H != W, tests/test_gpu_rect_maps.py): every row plans the loop
    form, tile and row order it records, per launch kind, and takes the host routes it records - so a heuristic change cannot quietly
    turn the rectangles into copies of one kernel family.  Rows that force a tile ask for one K slice and get it."""
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    from tests.helpers import RECT_CASES, RECT_WGRAD_ROW_CASES, assert_rect_wgrad_row_plan, epi_plan, rect_geom, rect_plan, tune_override
    assert len({c.name for c in RECT_CASES}) == len(RECT_CASES) >= 39
    bad = []
    for c in RECT_CASES:
        assert c.geom[1] != c.geom[2], c.name
        got = rect_plan(ops, c)
        if got != c.plan:
            bad.append((c.name, got, c.plan))
        g = rect_geom(ops, c)
        with tune_override(ops, g, c.tune):
            for kind, (_, split) in (c.tune or {}).items():
                assert epi_plan(g.shape(kind), {"fwd": 0, "dgrad": 1}[kind])[3] == split, c.name
    assert not bad, bad
    assert not ops._TUNE_OVERRIDE
    # every family the table is there for is reached: tap-major image-major and position-major, patch-resident in its four tiles
    fwd = {c.plan["fwd"] for c in RECT_CASES if "fwd" in c.plan}
    assert {(1, 64, 64, 0), (1, 128, 64, 0), (1, 64, 128, 0), (1, 128, 128, 0), (0, 64, 64, 0), (0, 128, 16, 0)} <= fwd
    assert sum(1 for p in fwd if p[3] > 0) >= 5
    assert {c.plan["route"][:2] for c in RECT_CASES} >= {("plain", "plain"), ("plain", "ups"), ("rows", "xfold"), ("rows", "t"), ("subpixel", "plain")}
    for case in RECT_WGRAD_ROW_CASES:      # the row-resident weight gradient and its refusals at W < 4
        assert_rect_wgrad_row_plan(case)
