"""Write tests/golden/ingest.npz by calling THE REFERENCE's process_pil_image (data_handling/img_datasets.py:296-303) on seeded
uint8 images: the fixtures that pin the PIL-exact resize of ingest.py / gim_resize_bilinear_u8.

Runs only where the reference tree and PIL are present (the reference's path: argv[1] or $GIM_REFERENCE); never imported by a test
or by the product.  torchvision (requirements.txt:14) need not be installed: the one transform the path touches, ToTensor, is
supplied here per its published behaviour (uint8 HWC -> float32 CHW / 255), like oracle/make_golden.py does; tqdm likewise.

Per case i the file holds
    c<i>/src   uint8 [H, W, C]      the seeded source image (C = 3: mode RGB, C = 1: mode L)
    c<i>/ref   float32 [C_out, S, S] what process_pil_image returned (after convert('L') where c<i>/gray is 1, as load_image does)
    c<i>/u8    uint8 [S, S, C_out]   the image behind that tensor, rint((ref + 1) * 127.5)
    c<i>/gray  0 / 1
and `names`, one label per case.

    python tools/make_ingest_golden.py /path/to/reference
"""
import os
import sys
import types

sys.dont_write_bytecode = True

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("GIM_REFERENCE", "")
if not os.path.isfile(os.path.join(REF, "data_handling", "img_datasets.py")):
    raise SystemExit("reference tree not found: pass its path")
sys.path.insert(0, REF)


class ToTensor:
    def __call__(self, pic):
        a = np.array(pic, dtype=np.uint8)
        if a.ndim == 2:
            a = a[:, :, None]
        return torch.from_numpy(a.transpose(2, 0, 1).copy()).float().div(255)


def _stand_ins():
    for name in ("torchvision", "tqdm"):
        try:
            __import__(name)
        except ImportError:
            mod = types.ModuleType(name)
            if name == "torchvision":
                tvt = types.ModuleType("torchvision.transforms")
                tvt.ToTensor = ToTensor
                mod.transforms = tvt
                sys.modules["torchvision.transforms"] = tvt
            else:
                mod.tqdm = lambda it, **kw: it
            sys.modules[name] = mod


# (label, H, W, source channels, S, convert('L') first, binary pixels)
CASES = [
    ("13x7_to_8_rgb", 13, 7, 3, 8, False, False),             # different tables per axis
    ("224x224_to_32_rgb", 224, 224, 3, 32, False, False),     # 17-tap rows
    ("105x105_to_32_gray_from_rgb", 105, 105, 3, 32, True, False),
    ("5x9_to_8_rgb", 5, 9, 3, 8, False, False),               # upscale, edge clamping
    ("8x20_to_8_rgb", 8, 20, 3, 8, False, False),             # horizontal pass only
    ("20x8_to_8_l", 20, 8, 1, 8, False, False),               # vertical pass only
    ("8x8_to_8_rgb", 8, 8, 3, 8, False, False),               # copy
    ("224x224_to_20_l", 224, 224, 1, 20, False, False),       # band tail: 20 is no multiple of the band height
    ("33x17_to_16_rgb_binary", 33, 17, 3, 16, False, True),   # the upper clamp
    ("1x5_to_4_rgb", 1, 5, 3, 4, False, False),               # degenerate source axis
]


def main():
    _stand_ins()
    import data_handling.img_datasets as ids
    rng = np.random.default_rng(20240607)
    out = {"names": np.asarray([c[0] for c in CASES])}
    for i, (name, H, W, C, S, gray, binary) in enumerate(CASES):
        src = rng.integers(0, 2, (H, W, C), dtype=np.uint8) * 255 if binary else rng.integers(0, 256, (H, W, C), dtype=np.uint8)
        pil = Image.fromarray(src[:, :, 0] if C == 1 else src)
        if gray:
            pil = pil.convert("L")           # load_image(img_mode='L'): before the resize
        ref = ids.process_pil_image(pil, img_size=S).numpy()
        u8 = np.rint((ref.astype(np.float64) + 1.0) * 127.5)
        assert u8.min() >= 0 and u8.max() <= 255 and ref.dtype == np.float32 and ref.shape == (1 if gray else C, S, S)
        out["c%d/src" % i] = src
        out["c%d/ref" % i] = ref
        out["c%d/u8" % i] = np.ascontiguousarray(u8.astype(np.uint8).transpose(1, 2, 0))
        out["c%d/gray" % i] = np.asarray(int(gray))
    path = os.path.join(OUT, "ingest.npz")
    np.savez_compressed(path, **out)
    print("ingest.npz: %d cases, %d bytes" % (len(CASES), os.path.getsize(path)))
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
