"""Seeded inputs of the KITTI 2015 flow / mask evaluation tests (tests/test_kitti_flow_eval.py) and of the fixture generator
tools/make_kitti_flow_golden.py, which records the reference's outputs for them in tests/golden/kitti_flow_eval.npz, plus a
writer of 16-bit RGB PNGs with a chosen filter type per row (forward filtering needs no serial loop).

The composition cases plant what test_mask.py:129-138 and mask_error branch on: mask products on both sides of 0.5, pixels where
flow_cam == flow_fwd exactly, one clear per-sample maximum of the flow difference, object ids above 1, and semantic labels both
26 (car) and not 26."""
import struct
import zlib

import numpy as np

THRESH = 0.94                           # test_mask.py:38
# (name, h, w, Hg, Wg, seed): a small case with a non-integer size ratio, and the protocol's 256x832 -> 375x1242
MASK_CASES = [("small", 24, 40, 37, 61, 51), ("kitti", 256, 832, 375, 1242, 52)]
# (name, H, W, seed): W < 64, W > 64 with H = 70 (rows in two waves), one row, exactly one wave, and H = 520 (the decoder
# handles bands of 512 rows: the last row of the first band is carried to the second)
PNG_CASES = [("narrow", 9, 7, 61), ("band", 70, 100, 62), ("row", 1, 65, 63), ("full_wave", 64, 3, 64), ("two_bands", 520, 5, 65)]
MAX_DIFF = 96.0


def compose_inputs(h, w, seed, B=1):
    """-> explainability_mask [B,4,h,w], flow_cam, flow_fwd [B,2,h,w] fp32"""
    r = np.random.RandomState(seed)
    mask = (r.rand(B, 4, h, w) * 0.5).astype(np.float32)               # 1 - (1-m1)(1-m2) in [0, 0.75]: both sides of 0.5
    cam = (r.randn(B, 2, h, w) * 12.0).astype(np.float32)
    mag = r.rand(B, 1, h, w) * 0.12 * MAX_DIFF                         # census: 1 - d/max > 0.94 <=> d < 0.06 max: about half
    ang = r.rand(B, 1, h, w) * 2 * np.pi
    fwd = (cam + np.concatenate([mag * np.cos(ang), mag * np.sin(ang)], 1)).astype(np.float32)
    same = r.rand(B, 1, h, w) < 0.05                                   # flow_cam == flow_fwd: soft = 1 exactly
    fwd = np.where(same, cam, fwd)
    for b in range(B):                                                 # one clear maximum per sample
        y, x = r.randint(h), r.randint(w)
        fwd[b, :, y, x] = cam[b, :, y, x] + np.array([MAX_DIFF * (1 + b), -MAX_DIFF * 0.5], np.float32)
    return mask, cam, fwd


def gt_maps(Hg, Wg, seed):
    """-> obj_map, semantic [Hg,Wg] uint8: blocks of object ids 0..3 and of labels 26 (car) / 7 / 21 / 24"""
    r = np.random.RandomState(seed + 1000)
    by, bx = (Hg + 7) // 8, (Wg + 7) // 8
    ids = r.choice([0, 0, 0, 1, 2, 3], size=(by, bx)).astype(np.uint8)
    lab = r.choice([26, 26, 7, 21, 24], size=(by, bx)).astype(np.uint8)
    up = lambda a: np.ascontiguousarray(np.repeat(np.repeat(a, 8, 0), 8, 1)[:Hg, :Wg])      # noqa: E731
    obj = up(ids)
    obj[r.rand(Hg, Wg) < 0.05] = 0                                     # holes, so that blocks are not uniform
    sem = up(lab)
    sem[r.rand(Hg, Wg) < 0.05] = 11
    return obj, sem


def flow_samples(H, W, seed):
    """-> [H,W,3] uint16 samples of a KITTI flow PNG: R = 64 u + 2^15, G = 64 v + 2^15, B = valid (flow_io.py:120-140), with
    zero rows, saturated samples and both byte values 0 and 255 present"""
    r = np.random.RandomState(seed)
    a = np.zeros((H, W, 3), dtype=np.uint16)
    a[..., :2] = np.clip(np.round(r.randn(H, W, 2) * 40.0 * 64.0) + 2 ** 15, 0, 65535).astype(np.uint16)
    a[..., 2] = r.rand(H, W) > 0.4
    a[r.rand(H, W) < 0.1] = 0
    a[r.rand(H, W) < 0.02, :2] = 65535
    a[r.rand(H, W) < 0.02, :2] = 255
    return a


def _paeth(a, b, c):
    a, b, c = a.astype(np.int32), b.astype(np.int32), c.astype(np.int32)
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def _chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xffffffff)


def encode_png(samples, filters=None, bit_depth=16, colour_type=2, interlace=0, idat_split=3):
    """PNG file bytes of samples [H,W,3] uint16 (most significant byte first) with filter type filters[y] on row y (default:
    cycling 0..4), the compressed stream cut into idat_split IDAT chunks.  bit_depth / colour_type / interlace only set the
    header fields (for the rejection tests)."""
    H, W, _ = samples.shape
    if filters is None:
        filters = np.arange(H) % 5
    raw = samples.astype(">u2").view(np.uint8).reshape(H, 6 * W).astype(np.int32)
    left = np.concatenate([np.zeros((H, 6), np.int32), raw[:, :-6]], 1) if W > 1 else np.zeros_like(raw)
    up = np.concatenate([np.zeros((1, 6 * W), np.int32), raw[:-1]], 0)
    upleft = np.concatenate([np.zeros((H, 6), np.int32), up[:, :-6]], 1) if W > 1 else np.zeros_like(raw)
    pred = [np.zeros_like(raw), left, up, (left + up) >> 1, _paeth(left, up, upleft)]
    out = np.empty((H, 1 + 6 * W), dtype=np.uint8)
    for y in range(H):
        out[y, 0] = filters[y]
        out[y, 1:] = (raw[y] - pred[int(filters[y])][y]) & 255
    z = zlib.compress(out.tobytes(), 1)
    cuts = [len(z) * k // idat_split for k in range(idat_split + 1)]
    ihdr = struct.pack(">IIBBBBB", W, H, bit_depth, colour_type, 0, 0, interlace)
    return b'\x89PNG\r\n\x1a\n' + _chunk(b'IHDR', ihdr) + b''.join(_chunk(b'IDAT', z[cuts[k]:cuts[k + 1]]) for k in range(idat_split)) + \
        _chunk(b'IEND', b'')
