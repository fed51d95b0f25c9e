"""csrc/roc.hip on the MI355X: the ROC count planes (ops.roc_counts), the eight-word record (ops.roc_record) and
authentication_eval.roc_statistics on CUDA tensors.  Everything is an integer count, so every comparison is exact equality, against a
numpy broadcast of the three definitions (for one large shape: binary searches in the sorted scores, themselves checked against the
broadcast) or against roc_statistics_host."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROC_TILE = 1024          # floats of one LDS tile of the counts kernel (csrc/roc.hip: ROC_TILE)
INF = float("inf")


def dev():
    return torch.device("cuda:0")


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev())


def _planes(cand, pos, neg):
    """The three definitions as numpy broadcasts of fp32 comparisons, in blocks of candidates."""
    out = np.empty((3, len(cand)), dtype=np.int64)
    step = max(1, (1 << 24) // max(len(pos), len(neg)))
    for i in range(0, len(cand), step):
        c = cand[i:i + step, None]
        out[0, i:i + step] = (pos[None, :] >= c).sum(1)
        out[1, i:i + step] = (neg[None, :] < c).sum(1)
        out[2, i:i + step] = (neg[None, :] == c).sum(1)
    return out


def _scores(rng, n, levels=0):
    """n fp32 scores: continuous, or drawn from `levels` distinct values (ties)."""
    if levels:
        return (rng.randint(0, levels, size=n) * 0.25 - 1.0).astype(np.float32)
    return rng.randn(n).astype(np.float32)


def _check_counts(cand, pos, neg):
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    got = ops.roc_counts(_gpu(cand), _gpu(pos), _gpu(neg))
    assert got.dtype == torch.int64 and tuple(got.shape) == (3, len(cand))
    assert np.array_equal(got.cpu().numpy(), _planes(cand, pos, neg))


# every n_cand edge and every score-count edge of the tiling appears in some row; candidates are a mix of scores (ties) and others
TILING = [(1, 1, 1), (63, 2, ROC_TILE - 1), (64, ROC_TILE, 2), (65, ROC_TILE + 1, 1), (257, 3 * ROC_TILE + 5, ROC_TILE - 1),
          (1, ROC_TILE - 1, ROC_TILE + 1), (64, 1, 3 * ROC_TILE + 5), (257, ROC_TILE, ROC_TILE)]


@pytest.mark.parametrize("n_cand,n_pos,n_neg", TILING)
@pytest.mark.parametrize("levels", [0, 8])
def test_counts_at_the_edges_of_the_tiling(n_cand, n_pos, n_neg, levels):
    rng = np.random.RandomState(n_cand * 7 + n_pos + 3 * n_neg)
    pos, neg = _scores(rng, n_pos, levels), _scores(rng, n_neg, levels)
    both = np.concatenate([pos, neg])
    cand = np.where(rng.rand(n_cand) < 0.5, both[rng.randint(0, len(both), size=n_cand)], _scores(rng, n_cand, levels)).astype(np.float32)
    _check_counts(cand, pos, neg)


@pytest.mark.parametrize("n_cand", [1, 65])
def test_counts_over_several_slices(n_cand):
    """One tile per slice; the positives' last tile, in a slice of its own, has 5 scores."""
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    n_pos, n_neg = 2 * ROC_TILE + 5, ROC_TILE
    assert ops.roc_slices(n_cand, n_pos + n_neg) == 4
    rng = np.random.RandomState(n_cand + n_pos)
    pos, neg = _scores(rng, n_pos, 8), _scores(rng, n_neg, 8)
    cand = np.concatenate([pos[-1:], _scores(rng, n_cand - 1, 8)]) if n_cand > 1 else neg[-1:]
    _check_counts(cand, pos, neg)


def _planes_sorted(cand, pos, neg):
    """The same counts from binary searches in the sorted fp32 scores (no NaN): for the one shape too large to broadcast."""
    sp, sn = np.sort(pos), np.sort(neg)
    lt = np.searchsorted(sn, cand, side="left")
    return np.stack([len(pos) - np.searchsorted(sp, cand, side="left"), lt, np.searchsorted(sn, cand, side="right") - lt]).astype(np.int64)


def test_counts_with_two_tiles_per_slice():
    """17 workgroups of candidates -> 241 slices for 252 tiles: two tiles per slice, 126 slices at work, the rest idle; one slice
    holds the positives' last tile (5 scores) and the negatives' first."""
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    n_cand, n_pos, n_neg = 4097, 150 * ROC_TILE + 5, 100 * ROC_TILE + 1
    assert ops.roc_slices(n_cand, n_pos + n_neg) == 241
    rng = np.random.RandomState(12)
    pos, neg = _scores(rng, n_pos, 8), _scores(rng, n_neg)
    cand = np.concatenate([pos[:2000], neg[:2000], _scores(rng, 97)])
    assert np.array_equal(_planes_sorted(cand[::64], pos, neg), _planes(cand[::64], pos, neg))       # the reference's reference
    got = ops.roc_counts(_gpu(cand), _gpu(pos), _gpu(neg))
    assert np.array_equal(got.cpu().numpy(), _planes_sorted(cand, pos, neg))


def test_slices_follow_the_candidate_count():
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    assert ops.roc_slices(1, 1) == ops.roc_slices(1, ROC_TILE) == 1 and ops.roc_slices(1, ROC_TILE + 1) == 2
    assert ops.roc_slices(256, 10 ** 6) == ops.roc_slices(257, 10 ** 6) == 977          # never more slices than tiles
    assert ops.roc_slices(256, 10 ** 7) == 4096 and ops.roc_slices(257, 10 ** 7) == 2048 and ops.roc_slices(200000, 200000) == 6
    with pytest.raises(RuntimeError):
        ops.roc_slices(0, 5)
    with pytest.raises(RuntimeError):
        ops.roc_slices(5, 2 ** 31)


# value classes: (pos, neg)
VALUES = {
    "all_equal": (np.full(70, 0.5), np.full(33, 0.5)),
    "eight_values": (_scores(np.random.RandomState(1), 300, 8), _scores(np.random.RandomState(2), 200, 8)),
    "infinities": (np.array([INF, 1., -INF, 0., INF]), np.array([-INF, INF, 2., -INF])),
    "signed_zero": (np.array([-0.0, 0.0, 1.0]), np.array([0.0, -0.0, -1.0, -0.0])),
    "subnormals": (np.array([1e-40, 2e-40, 0.]), np.array([2e-40, 0., 1e-40, 1e-40])),
    "one_positive": (np.array([0.25]), _scores(np.random.RandomState(3), 90)),
    "one_negative": (_scores(np.random.RandomState(4), 90), np.array([-0.25])),
    "1000_777": (_scores(np.random.RandomState(5), 1000), _scores(np.random.RandomState(6), 777) - 1.0),
    "1000_777_ties": (_scores(np.random.RandomState(7), 1000, 8), _scores(np.random.RandomState(8), 777, 8)),
}


@pytest.mark.parametrize("name", sorted(VALUES))
def test_counts_by_value_class(name):
    pos, neg = (v.astype(np.float32) for v in VALUES[name])
    assert name != "subnormals" or len(np.unique(pos)) == 3          # fp32 keeps them apart, and so must the kernel
    _check_counts(np.concatenate([pos, neg, np.float32([0.0, -0.0, INF, -INF, 1e-40])]), pos, neg)


@pytest.mark.parametrize("name", sorted(VALUES))
def test_record_and_statistics_equal_the_host_s(name):
    from optimalstrategiesagainstgenerativeattacks_amd import authentication_eval as ae
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    pos, neg = (v.astype(np.float32) for v in VALUES[name])
    n_pos, n_neg = len(pos), len(neg)
    want = ae.roc_statistics_host(pos, neg)
    got = ae.roc_statistics(_gpu(pos), _gpu(neg))
    assert got == want and [type(got[k]) for k in sorted(got)] == [type(want[k]) for k in sorted(want)]
    record, counts = ops.roc_record(_gpu(pos), _gpu(neg))
    planes = _planes(np.concatenate([pos, neg]), pos, neg)
    assert len(record) == ops.ROC_WORDS == 8 and all(type(w) is int for w in record)
    assert counts.dtype == torch.int32 and np.array_equal(counts.cpu().numpy(), planes)
    key = planes[0] * n_neg + planes[1] * n_pos
    i = record[3]
    assert record[0] == planes[1, :n_pos].sum() and record[1] == planes[2, :n_pos].sum()
    assert record[2] == key.max() == key[i] and record[4] == planes[0, i] and record[5] == planes[1, i] and record[6] == 0
    both = np.concatenate([pos, neg])
    assert record[7] == int(both[i:i + 1].view(np.uint32)[0])
    tied = both[key == key.max()]
    assert both[i] == tied.max() and i == np.flatnonzero((key == key.max()) & (both == tied.max()))[0]     # the tie rule


def test_two_calls_are_bit_identical():
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    rng = np.random.RandomState(9)
    pos, neg = _gpu(_scores(rng, 3 * ROC_TILE + 5, 8)), _gpu(_scores(rng, 2 * ROC_TILE + 1, 8))
    assert ops.roc_slices(pos.numel() + neg.numel(), pos.numel() + neg.numel()) > 1       # the slices meet in atomics
    r1, c1 = ops.roc_record(pos, neg)
    r2, c2 = ops.roc_record(pos, neg)
    assert r1 == r2 and torch.equal(c1, c2)
    assert torch.equal(ops.roc_counts(pos[:65], pos, neg), ops.roc_counts(pos[:65], pos, neg))
    assert torch.equal(ops.roc_counts(torch.cat([pos, neg]), pos, neg), c1.to(torch.int64))


def test_nan_scores_are_counted_and_refused():
    from optimalstrategiesagainstgenerativeattacks_amd import authentication_eval as ae
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    nan = float("nan")
    pos, neg = np.float32([1., nan, 0.5, nan]), np.float32([nan, 0.5, 0.])
    record, counts = ops.roc_record(_gpu(pos), _gpu(neg))
    assert record[6] == 3
    assert np.array_equal(counts.cpu().numpy(), _planes(np.concatenate([pos, neg]), pos, neg))     # a NaN compares false everywhere
    with pytest.raises(ValueError, match="NaN"):
        ae.roc_statistics(_gpu(pos), _gpu(neg))
    with pytest.raises(ValueError, match="NaN"):
        ae.roc_statistics(_gpu([1., 2.]), _gpu([nan]))
    with pytest.raises(ValueError, match="empty"):
        ae.roc_statistics(torch.zeros(0, device=dev()), _gpu([1.]))


def test_a_dirty_oversized_workspace_changes_nothing():
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    rng = np.random.RandomState(10)
    pos, neg = _gpu(_scores(rng, 1500, 8)), _gpu(_scores(rng, 700, 8))
    n = pos.numel() + neg.numel()
    record, counts = ops.roc_record(pos, neg)
    work = torch.full((3 * n + 1000,), 0x7f7f7f7f, device=dev(), dtype=torch.int32)
    record_w, counts_w = ops.roc_record(pos, neg, counts=work)
    assert record_w == record and torch.equal(counts_w, counts)
    assert counts_w.data_ptr() == work.data_ptr() and bool((work[3 * n:] == 0x7f7f7f7f).all())     # nothing past its own words


def test_views_and_bad_arguments():
    """Scores at any float offset of a buffer (no 16-byte alignment) and strided views count as their values do; CPU tensors, other
    dtypes, other ranks and a short workspace raise."""
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    rng = np.random.RandomState(11)
    buf = _scores(rng, 2 * ROC_TILE + 40, 8)
    g = _gpu(buf)
    for off in (1, 2, 3):
        pos, neg = buf[off:off + ROC_TILE + 3], buf[ROC_TILE + 7 + off:]
        got = ops.roc_counts(g[:65], g[off:off + ROC_TILE + 3], g[ROC_TILE + 7 + off:])
        assert np.array_equal(got.cpu().numpy(), _planes(buf[:65], pos, neg))
    got = ops.roc_counts(g[:65], g[::3], g[1::2])
    assert np.array_equal(got.cpu().numpy(), _planes(buf[:65], buf[::3], buf[1::2]))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.roc_counts(torch.zeros(3), g, g)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.roc_record(g, g.double())
    with pytest.raises(RuntimeError, match="1-D"):
        ops.roc_counts(g[:4], g[:8].view(2, 4), g)
    with pytest.raises(RuntimeError, match="1-D"):
        ops.roc_record(g[:0], g)
    with pytest.raises(RuntimeError, match="workspace"):
        ops.roc_record(g[:4], g[:4], counts=torch.zeros(23, device=dev(), dtype=torch.int32))
