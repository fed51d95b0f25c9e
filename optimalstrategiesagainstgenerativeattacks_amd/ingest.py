"""From image files to the resident episode bank: the step in front of ``data.EpisodeBank``.

The reference's loaders (data_handling/img_datasets.py:284-303, ``load_image`` -> ``process_pil_image``) decode a file, optionally
``convert('L')``, and ``resize((S, S), Image.BILINEAR)`` it - per image, per access.  Here the files are decoded ONCE on the host into
an ``ImagePack`` of native-size uint8 images (no resize), and ``ImagePack.to_bank`` resizes the whole pack on the GPU
(``gim_resize_bilinear_u8``) into the S x S bank, so one pack serves every image size.  The resize is PIL's, bit for bit: BILINEAR
in PIL is an antialiased two-pass resampler (support scaled by the shrink factor, 22-bit fixed-point weights, the horizontal
result rounded to uint8 before the vertical pass), which no two-tap "bilinear" reproduces when shrinking.  The weights are computed
here in double precision (``resample_table``); the device side is integer only.
"""
import functools
import math
import os

import numpy as np
import torch

from . import _lib
from ._lib import check

PRECISION_BITS = 22                    # PIL: 32 - 8 - 2
OMNIGLOT_SUFFIXES = ('.png', '.jpg', 'jpeg', '.JPG', 'JPEG')     # data_handling/img_datasets.py:144


@functools.lru_cache(maxsize=None)
def _resample_table(in_size, out_size):
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = fs                       # the triangle filter's support (1.0) times the filter scale
    ksize = 2 * int(math.ceil(support)) + 1
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    coef = np.zeros((out_size, ksize), dtype=np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)                  # int(): C truncation
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = []
        for x in range(xmax):
            t = abs((x + xmin - center + 0.5) / fs)
            w.append(1.0 - t if t < 1.0 else 0.0)
        ww = 0.0
        for v in w:                                                 # summed in tap order, as the C loop does
            ww += v
        for x in range(xmax):
            v = w[x] / ww if ww != 0.0 else w[x]
            coef[xx, x] = int(0.5 + v * (1 << PRECISION_BITS))      # weights are >= 0
        bounds[xx] = (xmin, xmax)
    bounds.setflags(write=False)
    coef.setflags(write=False)
    return bounds, coef


def resample_table(in_size, out_size):
    """PIL's BILINEAR coefficient table of one axis: ``(bounds int32 [out, 2], coef int32 [out, ksize])`` with
    ``bounds[i] = (first source index, tap count)`` and 22-bit fixed-point weights (unused taps 0); ``None`` when the axis keeps
    its size (PIL skips that pass: a copy, not a pass with unit weights).  Depends on (in, out) only; cached, read-only arrays."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError("resample_table: sizes must be positive, got %d -> %d" % (in_size, out_size))
    if in_size == out_size:
        return None
    return _resample_table(in_size, out_size)


_device_tables = {}


def _device_table(in_size, out_size, device):
    """(bounds pointer, coef pointer, ksize) of the axis on `device`; (None, None, 0) for a copied axis."""
    tab = resample_table(in_size, out_size)
    if tab is None:
        return None, None, 0
    key = (in_size, out_size, str(device))
    if key not in _device_tables:
        _device_tables[key] = tuple(torch.from_numpy(np.array(t)).to(device) for t in tab)
    b, c = _device_tables[key]
    return b.data_ptr(), c.data_ptr(), c.shape[1]


def _size_pair(size):
    return (int(size), int(size)) if np.isscalar(size) else (int(size[0]), int(size[1]))


def resize_images(images_u8, size, to_gray=False, out=None):
    """uint8 [N, H, W, C] (CUDA, contiguous, C = 1 or 3) -> uint8 [N, S, S, C_out]: ``Image.resize((S, S), Image.BILINEAR)`` of
    every image, after ``convert('L')`` with ``to_gray`` (C = 3 -> C_out = 1).  ``size`` = S or (out_h, out_w); ``out``: a
    contiguous CUDA uint8 tensor of the result's shape to write into (e.g. rows of a bank)."""
    if not (torch.is_tensor(images_u8) and images_u8.is_cuda):
        raise RuntimeError("resize_images: images must be a CUDA uint8 [N, H, W, C] tensor (no CPU path)")
    if not (images_u8.dtype == torch.uint8 and images_u8.dim() == 4 and images_u8.is_contiguous()):
        raise RuntimeError("resize_images: images must be a contiguous uint8 [N, H, W, C] tensor")
    N, H, W, C = images_u8.shape
    out_h, out_w = _size_pair(size)
    c_out = 1 if to_gray else C
    if out is None:
        out = torch.empty((N, out_h, out_w, c_out), device=images_u8.device, dtype=torch.uint8)
    elif not (out.is_cuda and out.device == images_u8.device and out.dtype == torch.uint8 and out.is_contiguous()
              and tuple(out.shape) == (N, out_h, out_w, c_out)):
        raise RuntimeError("resize_images: out must be a contiguous uint8 %s tensor on %s" % ((N, out_h, out_w, c_out), images_u8.device))
    if N == 0:
        return out
    xb, xc, xk = _device_table(W, out_w, images_u8.device)
    yb, yc, yk = _device_table(H, out_h, images_u8.device)
    check(_lib.load().gim_resize_bilinear_u8(images_u8.data_ptr(), N, H, W, C, int(bool(to_gray)), out.data_ptr(), out_h, out_w,
                                             xb, xc, xk, yb, yc, yk, torch.cuda.current_stream().cuda_stream), "resize_bilinear_u8")
    return out


class ImagePack:
    """Host container of decoded, NATIVE-size uint8 images (HWC), images of one class contiguous:
    ``data`` flat uint8 bytes, ``shapes`` int32 [n, 3] = (H, W, C), ``byte_offsets`` int64 [n + 1] into ``data``,
    ``class_offsets`` int64 [n_classes + 1] into the images, ``class_names`` unicode [n_classes].  Nothing is filtered: a class
    with fewer than m + n + k images stays in the pack and is dropped by ``EpisodeSampler``, as the reference's dataset drops it."""

    def __init__(self, data, shapes, byte_offsets, class_offsets, class_names):
        self.data = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
        self.shapes = np.asarray(shapes, dtype=np.int32).reshape(-1, 3)
        self.byte_offsets = np.asarray(byte_offsets, dtype=np.int64)
        self.class_offsets = np.asarray(class_offsets, dtype=np.int64)
        self.class_names = np.asarray(class_names, dtype=np.str_)
        n = len(self.shapes)
        sizes = self.shapes.astype(np.int64).prod(axis=1)
        if not (len(self.byte_offsets) == n + 1 and np.array_equal(np.diff(self.byte_offsets), sizes)
                and self.byte_offsets[0] == 0 and self.byte_offsets[-1] == self.data.size):
            raise ValueError("ImagePack: byte_offsets do not match shapes / data")
        if not (len(self.class_offsets) == len(self.class_names) + 1 and self.class_offsets[0] == 0 and self.class_offsets[-1] == n
                and (np.diff(self.class_offsets) >= 0).all()):
            raise ValueError("ImagePack: class_offsets do not match class_names / the image count")

    @classmethod
    def from_images(cls, images_per_class, class_names):
        """images_per_class: per class a list of uint8 arrays [H, W] or [H, W, C]."""
        flat, shapes, class_offsets = [], [], [0]
        for imgs in images_per_class:
            for a in imgs:
                a = np.asarray(a, dtype=np.uint8)
                a = a[:, :, None] if a.ndim == 2 else a
                flat.append(a.reshape(-1))
                shapes.append(a.shape)
            class_offsets.append(len(shapes))
        sizes = [f.size for f in flat]
        data = np.concatenate(flat) if flat else np.zeros(0, dtype=np.uint8)
        return cls(data, np.asarray(shapes, dtype=np.int32).reshape(-1, 3), np.concatenate([[0], np.cumsum(sizes, dtype=np.int64)]),
                   class_offsets, list(class_names))

    def __len__(self):
        return len(self.shapes)

    def image(self, i):
        """Image i as a uint8 [H, W, C] view."""
        return self.data[self.byte_offsets[i]:self.byte_offsets[i + 1]].reshape(tuple(self.shapes[i]))

    def save(self, path):
        """One .npz of plain arrays (class names as a unicode array: it loads with allow_pickle=False)."""
        with open(path, "wb") as f:
            np.savez(f, data=self.data, shapes=self.shapes, byte_offsets=self.byte_offsets, class_offsets=self.class_offsets,
                     class_names=self.class_names)

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            return cls(z["data"], z["shapes"], z["byte_offsets"], z["class_offsets"], z["class_names"])

    def to_bank(self, img_size, img_channels, device, chunk_bytes=256 << 20):
        """The uint8 [n, S, S, img_channels] bank on `device`: every image resized as the reference's loader resizes it.  Runs of
        consecutive images of equal shape are uploaded in chunks of at most `chunk_bytes` (at least one image) and resized
        one launch per chunk straight into the bank's rows.  img_channels == 1 on an RGB pack converts to grayscale first
        (``load_image(img_mode='L')``); img_channels == 3 on a one-channel pack raises."""
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("ImagePack.to_bank: the bank lives on the GPU, device must be a CUDA device (no CPU path)")
        n = len(self)
        chans = np.unique(self.shapes[:, 2])
        if n == 0 or len(chans) != 1 or int(chans[0]) not in (1, 3):
            raise ValueError("ImagePack.to_bank: the pack must hold images of one channel count, 1 or 3 (has %s)" % chans.tolist())
        C = int(chans[0])
        if img_channels not in (1, 3):
            raise ValueError("ImagePack.to_bank: img_channels must be 1 or 3")
        if img_channels == 3 and C == 1:
            raise ValueError("ImagePack.to_bank: img_channels == 3 on a one-channel ('L') pack")
        to_gray = img_channels == 1 and C == 3
        bank = torch.empty((n, img_size, img_size, img_channels), device=device, dtype=torch.uint8)
        change = np.nonzero((np.diff(self.shapes, axis=0) != 0).any(axis=1))[0] + 1
        starts = np.concatenate([[0], change, [n]])
        for lo, hi in zip(starts[:-1], starts[1:]):
            H, W, _ = (int(v) for v in self.shapes[lo])
            per = max(1, int(chunk_bytes) // (H * W * C))
            for a in range(lo, hi, per):
                b = min(a + per, hi)
                host = torch.from_numpy(self.data[self.byte_offsets[a]:self.byte_offsets[b]]).view(b - a, H, W, C)
                resize_images(host.to(device), img_size, to_gray, out=bank[a:b])
        return bank


def _list_dirs(path):
    return sorted(d for d in os.listdir(path) if os.path.isdir(os.path.join(path, d)))


def _decode_classes(data_dir, class_dirs, keep_file, mode):
    try:
        from PIL import Image
    except ImportError as e:
        raise RuntimeError("packing a directory decodes image files with PIL (Pillow), which is not installed; decoding is the one "
                           "step that stays on the host") from e
    per_class = []
    for d in class_dirs:
        cls_dir = os.path.join(data_dir, d)
        imgs = []
        for f in sorted(f for f in os.listdir(cls_dir) if keep_file(cls_dir, f)):
            with Image.open(os.path.join(cls_dir, f), mode='r') as im:
                imgs.append(np.asarray(im.convert(mode), dtype=np.uint8))
        per_class.append(imgs)
    return ImagePack.from_images(per_class, class_dirs)


def pack_directory(root, split, img_suffix='.jpg', hierarchical=False, mode='RGB'):
    """Pack the tree ``ImgGIMDataSet`` reads (data_handling/img_datasets.py:48-62, 75-78): ``root/split/<class>/*<img_suffix>``,
    or with ``hierarchical`` ``root/split/<parent>/<class>/...`` (class name "parent/class").  Files are kept by
    ``name.endswith(img_suffix)``, decoded with ``Image.open(..).convert(mode)`` and stored at their native size.
    Classes and files are taken in SORTED order; the reference takes them in ``os.listdir`` order, which is arbitrary, so class
    indices agree with the reference's only up to that permutation (class names identify them)."""
    data_dir = os.path.join(root, split)
    if hierarchical:
        class_dirs = [os.path.join(p, d) for p in _list_dirs(data_dir) for d in _list_dirs(os.path.join(data_dir, p))]
    else:
        class_dirs = _list_dirs(data_dir)
    return _decode_classes(data_dir, class_dirs, lambda cls_dir, f: f.endswith(img_suffix), mode)


def pack_omniglot(root, split):
    """Pack the tree ``OmniglotGIMDataSet`` reads (data_handling/img_datasets.py:141-145): ``root/split/<alphabet>/<character>/``,
    regular files ending in the reference's suffix tuple, mode 'L'; class names are "alphabet/character".  Sorted order, as in
    ``pack_directory``."""
    data_dir = os.path.join(root, split)
    class_dirs = [os.path.join(a, c) for a in _list_dirs(data_dir) for c in _list_dirs(os.path.join(data_dir, a))]
    return _decode_classes(data_dir, class_dirs,
                           lambda cls_dir, f: os.path.isfile(os.path.join(cls_dir, f)) and f.endswith(OMNIGLOT_SUFFIXES), 'L')
