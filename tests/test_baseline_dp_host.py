"""Host side of data-parallel baseline training (baseline_training.py): the samplers' rank slices, the dropout counter's tiling over
ranks and iterations, and the argument checks of the new library entries.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gim_bn_stats_record", "gim_bn_stats_merge", "gim_bn_bwd_dx_total", "gim_bn_pool_bwd_dx_total")


class _Bank:
    """What the samplers read of a data.EpisodeBank; gather records its arguments and returns a tensor that names them."""

    def __init__(self, sizes, mirror=True):
        self.offsets, self.mirror = np.concatenate([[0], np.cumsum(sizes)]), mirror
        self.calls = []

    def gather(self, idx, flip):
        import torch
        idx, flip = np.asarray(idx), np.asarray(flip)
        assert idx.shape == flip.shape
        self.calls.append((idx.copy(), flip.copy()))
        return torch.from_numpy(idx.reshape(-1).astype(np.float32) * 2 + flip.reshape(-1))[:, None, None, None]


SIZES = [6, 1, 4, 1, 9, 2]


@pytest.mark.parametrize("world", [1, 2, 4])
def test_pair_sampler_rank_slices_concatenate_to_the_global_draw(world):
    from optimalstrategiesagainstgenerativeattacks_amd.baseline_training import PairSampler
    bank = _Bank(SIZES)
    s = PairSampler(bank, 12, seed=3)      # n_pos = 6: at world 4 rank 0 is all positives, rank 1 mixed, ranks 2 and 3 have none
    for it in (0, 5):
        idx, flip, _ = s.draw(it)
        parts, n_pos = [], []
        for rank in range(world):
            x1, x2, n = s.batch(it, rank, world)
            got_idx, got_flip = bank.calls[-1]
            assert got_idx.shape == (2, 12 // world)       # all first images, then all second images
            assert x1.shape[0] == x2.shape[0] == 12 // world
            parts.append((got_idx.T, got_flip.T))
            n_pos.append(n)
        assert np.array_equal(np.concatenate([p[0] for p in parts]), idx) and np.array_equal(np.concatenate([p[1] for p in parts]), flip)
        assert sum(n_pos) == s.n_pos == 6
        assert n_pos == {1: [6], 2: [6, 0], 4: [3, 3, 0, 0]}[world]
    # the default arguments are the single-process batch
    x1, x2, n = s.batch(5)
    assert np.array_equal(bank.calls[-1][0], s.draw(5)[0].T) and n == 6 and x1.shape[0] == 12


def test_pair_sampler_ranks_with_all_and_with_no_positives():
    from optimalstrategiesagainstgenerativeattacks_amd.baseline_training import PairSampler
    s = PairSampler(_Bank(SIZES), 8, seed=1)      # n_pos = 4, three rows per ... 8 / 4 = 2 rows per rank
    assert [s.batch(0, r, 4)[2] for r in range(4)] == [2, 2, 0, 0]
    s = PairSampler(_Bank(SIZES), 6, seed=1)      # n_pos = 3, two rows per rank: the middle rank has one of each
    assert [s.batch(0, r, 3)[2] for r in range(3)] == [2, 1, 0]


@pytest.mark.parametrize("world", [1, 2, 4])
def test_identity_sampler_rank_slices_concatenate_to_the_global_draw(world):
    from optimalstrategiesagainstgenerativeattacks_amd.baseline_training import IdentitySampler
    bank = _Bank(SIZES)
    s = IdentitySampler(bank, 8, seed=9)
    for it in (0, 7):
        idx, flip, label = s.draw(it)
        got = []
        for rank in range(world):
            x, lab = s.batch(it, rank, world)
            assert x.shape[0] == 8 // world and lab.dtype.is_floating_point is False and tuple(lab.shape) == (8 // world,)
            got.append(bank.calls[-1] + (lab.numpy(),))
        for k, ref in enumerate((idx, flip, label)):
            assert np.array_equal(np.concatenate([g[k] for g in got]), ref), (it, k)


def test_samplers_refuse_a_batch_the_ranks_cannot_share():
    from optimalstrategiesagainstgenerativeattacks_amd.baseline_training import IdentitySampler, PairSampler
    for s in (PairSampler(_Bank(SIZES), 10, seed=3), IdentitySampler(_Bank(SIZES), 10, seed=3)):
        with pytest.raises(ValueError, match="multiple of world"):
            s.batch(0, 0, 4)
        with pytest.raises(ValueError, match="rank"):
            s.batch(0, 2, 2)
        assert not s.bank.calls      # refused before anything is gathered
        s.batch(0, 1, 2)


def test_dropout_offsets_tile_the_global_counter():
    """Iteration `it` owns [it * N, (it + 1) * N), N the global element count; the ranks' ranges tile it in rank order without gaps
    or overlaps, and one rank is what the single-process trainer always did (it * numel)."""
    from optimalstrategiesagainstgenerativeattacks_amd.baseline_training import dropout_offset
    for world, numel in ((1, 4 * 2 * 2 * 512), (2, 4 * 2 * 2 * 512), (4, 2048), (3, 12)):
        n_global = world * numel
        for it in (0, 1, 3, 10 ** 6):
            starts = [dropout_offset(it, numel, r, world) for r in range(world)]
            assert starts[0] == it * n_global
            assert all(b - a == numel for a, b in zip(starts, starts[1:]))
            assert starts[-1] + numel == (it + 1) * n_global == dropout_offset(it + 1, numel, 0, world)
    assert dropout_offset(7, 4096) == 7 * 4096
    assert isinstance(dropout_offset(np.int64(3), np.int64(8), 1, 2), int)


def test_new_entry_points_are_declared_bound_and_exported():
    from optimalstrategiesagainstgenerativeattacks_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "gim_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.SIGNATURES, name
    for name in ("bn_stats_record", "bn_stats_merge", "DistSync", "default_sync", "bn_bwd_dx", "bn_pool_bwd_dx"):
        assert hasattr(ops, name), name
    assert ops.default_sync() is None      # no process group: the single-process path


def test_new_entries_check_their_arguments_before_any_launch():
    """Bad sizes and NULL pointers only: the new entries check their sizes before their device pointers, so every call here is
    refused on the host with no address for a kernel to touch."""
    import __graft_entry__
    from optimalstrategiesagainstgenerativeattacks_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        __graft_entry__.build()
    lib = _lib.load()
    n = None

    def counts(*v):
        return (ctypes.c_int64 * len(v))(*v)

    def merge(c, R, C, momentum=0.1, eps=1e-5):
        return lib.gim_bn_stats_merge(n, c, R, C, n, n, n, n, n, momentum, eps, n)

    for what, call, msg in (
            ("record: null pointers", lambda: lib.gim_bn_stats_record(n, n, n, 16, 8, n), b"null pointer"),
            ("record: no rows", lambda: lib.gim_bn_stats_record(n, n, n, 0, 8, n), b"bad dims"),
            ("record: C % 4", lambda: lib.gim_bn_stats_record(n, n, n, 16, 6, n), b"bad dims"),
            ("merge: null pointers", lambda: merge(counts(2, 2), 2, 8), b"null pointer"),
            ("merge: null counts", lambda: merge(n, 2, 8), b"null pointer"),
            ("merge: one row in all", lambda: merge(counts(1), 1, 8), b"at least two rows"),
            ("merge: a zero count", lambda: merge(counts(4, 0, 4), 3, 8), b"at least 1"),
            ("merge: a negative count", lambda: merge(counts(4, -1), 2, 8), b"at least 1"),
            ("merge: R = 65", lambda: merge(counts(*([2] * 65)), 65, 8), b"R <= 64"),
            ("merge: R = 0", lambda: merge(counts(2), 0, 8), b"R <= 64"),
            ("merge: C % 4", lambda: merge(counts(2, 2), 2, 6), b"bad dims"),
            ("merge: momentum", lambda: merge(counts(2, 2), 2, 8, momentum=1.5), b"momentum"),
            ("dx_total: null pointers", lambda: lib.gim_bn_bwd_dx_total(n, n, n, n, n, n, n, n, n, n, 16, 32, 8, n), b"null pointer"),
            ("dx_total: fewer rows in all than here", lambda: lib.gim_bn_bwd_dx_total(n, n, n, n, n, n, n, n, n, n, 16, 15, 8, n), b"M_total"),
            ("pool dx_total: null pointers", lambda: lib.gim_bn_pool_bwd_dx_total(n, n, n, n, n, n, n, n, n, 2, 4, 4, 8, 64, n), b"null pointer"),
            ("pool dx_total: fewer rows in all than here", lambda: lib.gim_bn_pool_bwd_dx_total(n, n, n, n, n, n, n, n, n, 2, 4, 4, 8, 31, n),
             b"M_total")):
        assert call() < 0, what
        assert msg in lib.gim_last_error(), (what, lib.gim_last_error())
    # 64 ranks are within the limit: the call gets as far as its device pointers
    assert merge(counts(*([1] * 64)), 64, 8) < 0 and b"null pointer" in lib.gim_last_error()
    # the parents keep their signatures and their refusals
    assert lib.gim_bn_bwd_dx(n, n, n, n, n, n, n, n, n, n, 16, 8, n) < 0 and b"bn_bwd_dx" in lib.gim_last_error()
    assert lib.gim_bn_pool_bwd_dx(n, n, n, n, n, n, n, n, n, 2, 4, 4, 8, n) < 0 and b"bn_pool_bwd_dx" in lib.gim_last_error()


def test_trainers_take_no_sync_without_a_process_group():
    from optimalstrategiesagainstgenerativeattacks_amd import baselines as bl
    from optimalstrategiesagainstgenerativeattacks_amd.baseline_training import SiameseTrainer
    enc = bl.ProtonetEmbeddingNet(1, 32)
    tr = SiameseTrainer(bl.SiameseNet(enc, enc.embedding_dim))
    assert tr.sync is None

    class Sync:
        rank, world = 1, 2
    assert SiameseTrainer(bl.SiameseNet(enc, enc.embedding_dim), sync=Sync).sync is Sync
