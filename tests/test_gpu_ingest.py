"""gim_resize_bilinear_u8 and the pack -> bank path on the GPU.  Every comparison is exact: the arithmetic is integer.  Expected
values: the reference's own process_pil_image results (tests/golden/data.npz resize/*, tests/golden/ingest.npz) and the numpy
restatement of tests/ingest_ref.py, which tests/test_ingest_host.py pins to those fixtures and to PIL."""
import os

import numpy as np
import pytest
import torch

from optimalstrategiesagainstgenerativeattacks_amd import ingest
from optimalstrategiesagainstgenerativeattacks_amd.data import EpisodeBank, OmniglotEpisodeBank
from tests import ingest_ref as ir

pytestmark = pytest.mark.gpu

CASES = ir.ingest_cases()


def dev():
    return torch.device("cuda:0")


def gpu_resize(src_np, size, gray=False):
    return ingest.resize_images(torch.from_numpy(np.ascontiguousarray(src_np)).to(dev()), size, gray).cpu().numpy()


def test_resize_then_gather_reproduces_process_pil_image(golden_dir):
    """The reference's process_pil_image end to end: data.npz resize/in (12x12x3) -> resize_images -> EpisodeBank.gather equals
    resize/out (the float tensor the reference returned at img_size = 8) bit for bit."""
    with np.load(os.path.join(golden_dir, "data.npz")) as z:
        src, want = z["resize/in"], z["resize/out"]
    bank = ingest.resize_images(torch.from_numpy(src[None]).to(dev()), 8)
    assert bank.shape == (1, 8, 8, 3) and bank.dtype == torch.uint8
    got = EpisodeBank(bank, [0, 1], 0, 1, 0, mirror=False).gather([0], [0]).cpu().numpy()[0]
    assert got.dtype == want.dtype and np.array_equal(got, want)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_ingest_fixture_cases(case):
    _, src, gray, _, u8 = case
    assert np.array_equal(gpu_resize(src[None], u8.shape[0], gray)[0], u8)


# (N, H, W, C, gray, out_h, out_w)
SWEEP = [
    (1, 4, 4, 3, False, 2, 2), (3, 4, 4, 3, False, 2, 2),
    (70000, 4, 4, 3, False, 2, 2),          # image index past 65 535: more (image, band) items than workgroups in the launch
    (3, 13, 7, 3, False, 8, 8),
    (2, 17, 23, 1, False, 5, 6),            # output rows of 6, 7, 15 bytes: the byte-wise vertical pass
    (2, 31, 45, 3, True, 9, 7),
    (2, 64, 48, 3, False, 10, 5),
    (2, 224, 224, 3, False, 64, 64),        # two bands per image, 9-tap windows
    (3, 105, 105, 1, False, 32, 32),
    (1, 300, 200, 3, False, 128, 128),      # several bands, tail band
    (2, 224, 224, 3, True, 128, 128),
    (1, 9, 9, 3, False, 20, 20),            # upscale
    (1, 500, 40, 3, False, 4, 16),          # 251-tap columns: bands of one or two rows
    (2, 6, 3000, 3, False, 6, 64),          # 9000-byte source rows: one row per staging chunk; no vertical pass
    (2, 40, 1500, 1, False, 8, 1500),       # ten rows per staging chunk; no horizontal pass
    (5, 16, 16, 3, True, 16, 16),           # grayscale conversion only
]


@pytest.mark.parametrize("shape", SWEEP, ids=["%dx%dx%dx%d%s_to_%dx%d" % (s[0], s[1], s[2], s[3], "g" if s[4] else "", s[5], s[6]) for s in SWEEP])
def test_sweep_against_numpy_restatement(shape):
    N, H, W, C, gray, oh, ow = shape
    rng = np.random.default_rng(sum(int(v) * 131 ** i for i, v in enumerate(shape)) % (1 << 31))
    src = rng.integers(0, 256, (N, H, W, C), dtype=np.uint8)
    src[0][src[0] < 128] = 0                # one image of extremes: rounded weights summing past 2^22 need the upper clamp
    src[0][src[0] >= 128] = 255
    got = gpu_resize(src, (oh, ow), gray)
    assert got.shape == (N, oh, ow, 1 if gray else C)
    assert np.array_equal(got, ir.resize(src, oh, ow, gray))


@pytest.mark.parametrize("guard", [4096, 4093])      # 4093: a destination that is not 4-byte aligned (byte-wise stores)
def test_guard_rows_stay_intact_and_runs_are_identical(guard):
    rng = np.random.default_rng(guard)
    N, H, W, S = 5, 57, 91, 24
    src_np = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    src = torch.from_numpy(src_np).to(dev())
    n = N * S * S * 3
    buf = torch.full((guard + n + guard,), 0xA5, dtype=torch.uint8, device=dev())
    out = buf[guard:guard + n].view(N, S, S, 3)
    ingest.resize_images(src, S, out=out)
    assert bool((buf[:guard] == 0xA5).all()) and bool((buf[guard + n:] == 0xA5).all())
    again = ingest.resize_images(src, S)
    assert torch.equal(out, again)
    assert np.array_equal(again.cpu().numpy(), ir.resize(src_np, S, S))


def test_offsets_beyond_2_31():
    """15 000 images of 224x224x3 = 2.26 GB in ONE launch: the last ten results equal a launch on those ten images alone."""
    N = 15000
    g = torch.Generator(device=dev()).manual_seed(3)
    src = torch.randint(0, 256, (N, 224, 224, 3), dtype=torch.uint8, device=dev(), generator=g)
    assert src.numel() > (1 << 31)
    out = ingest.resize_images(src, 16)
    tail = ingest.resize_images(src[N - 10:].clone(), 16)
    assert torch.equal(out[N - 10:], tail)
    assert np.array_equal(tail[-1].cpu().numpy(), ir.resize(src[N - 1].cpu().numpy(), 16, 16))


def test_argument_errors():
    with pytest.raises(RuntimeError, match="staging buffer"):
        ingest.resize_images(torch.zeros((1, 2, 6000, 3), dtype=torch.uint8, device=dev()), (2, 8))
    with pytest.raises(RuntimeError, match="shrink factor too large"):       # 600 rows x 400 x 3 bytes for ONE output row
        ingest.resize_images(torch.zeros((1, 600, 8, 3), dtype=torch.uint8, device=dev()), (2, 400))
    with pytest.raises(RuntimeError, match="C_in must be 1 or 3"):
        ingest.resize_images(torch.zeros((1, 8, 8, 2), dtype=torch.uint8, device=dev()), 4)
    with pytest.raises(RuntimeError, match="to_gray needs"):
        ingest.resize_images(torch.zeros((1, 8, 8, 1), dtype=torch.uint8, device=dev()), 4, to_gray=True)


def _mixed_pack(rng):
    shapes = {"a": [(12, 12)] * 5 + [(13, 7)] * 4, "b": [(13, 7)] * 2 + [(224, 224)] * 7, "c": [(224, 224)] * 2 + [(12, 12)] * 3}
    per_class = [[rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes[c]] for c in sorted(shapes)]
    return ingest.ImagePack.from_images(per_class, sorted(shapes))


def test_to_bank_of_a_mixed_pack_equals_per_image_resize():
    pack = _mixed_pack(np.random.default_rng(11))
    for channels in (3, 1):
        bank = pack.to_bank(16, channels, dev(), chunk_bytes=4 * 224 * 224 * 3)      # the nine 224x224 images: chunks of 4, 4, 1
        assert bank.shape == (len(pack), 16, 16, channels)
        for i in range(len(pack)):
            one = ingest.resize_images(torch.from_numpy(pack.image(i)[None].copy()).to(dev()), 16, to_gray=channels == 1)
            assert torch.equal(bank[i], one[0]), (channels, i)
    tiny = pack.to_bank(16, 3, dev(), chunk_bytes=1)                                 # smaller than any image: one image per launch
    assert torch.equal(tiny, pack.to_bank(16, 3, dev()))
    gray_pack = ingest.ImagePack.from_images([[np.zeros((5, 5), np.uint8)] * 3], ["x"])
    with pytest.raises(ValueError, match="img_channels == 3"):
        gray_pack.to_bank(8, 3, dev())


def test_from_pack_serves_the_episode_contract():
    pack = _mixed_pack(np.random.default_rng(12))
    m, n, k, S = 1, 3, 2, 16
    ds = EpisodeBank.from_pack(pack, S, m, n, k, device=dev(), example_cnt_per_class=2, seed=1)
    assert ds.n_classes == 2 and ds.class_ids.tolist() == [0, 1] and len(ds) == 4      # class "c": 5 images < m + n + k
    assert torch.equal(ds.bank, pack.to_bank(S, 3, dev()))
    ex = ds[3]
    assert ex["class"] == 1 and ex["class_name"] == "b"
    assert ex["leaked_sample"].shape == (m, 3, S, S) and ex["real_sample"].shape == (n, 3, S, S) and ex["si_sample"].shape == (k, 3, S, S)
    x = torch.cat([ex["leaked_sample"], ex["real_sample"], ex["si_sample"]])
    assert x.dtype == torch.float32 and float(x.min()) >= -1.0 and float(x.max()) <= 1.0
    gray = EpisodeBank.from_pack(pack, S, m, n, k, img_channels=1, device=dev())
    assert gray[0]["real_sample"].shape == (n, 1, S, S)
    om_pack = ingest.ImagePack.from_images([[np.full((105, 105), 7 * j, np.uint8) for j in range(20)]] * 2, ["A/c1", "A/c2"])
    om = OmniglotEpisodeBank.from_pack(om_pack, 32, 1, 5, 5, device=dev())
    ex = om[1]
    assert ex["class_name"] == "A/c2" and ex["si_sample"].shape == (5, 1, 32, 32) and not om.mirror
    with pytest.raises(ValueError):
        OmniglotEpisodeBank.from_pack(om_pack, 32, 10, 10, 1, device=dev())
