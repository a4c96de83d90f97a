"""NumPy restatement of the KITTI 2015 flow / mask evaluation entries (cc_amd/csrc/kitti_flow_eval.hip): the rigidity
composition of test_mask.py:129-138, mask_error (test_mask.py:224-262) with scipy.ndimage.zoom(order=0) written out as an index
lookup, and a slow PNG unfilter written from the PNG specification (section 9, "Filtering").  Pinned against the reference-written
fixture tests/golden/kitti_flow_eval.npz by tests/test_kitti_flow_eval.py; the GPU tests compare the kernels with it."""
import numpy as np


def compose_norm(exp_mask, flow_cam, flow_fwd, thresh):
    """-> (bare, census, combined) [B,1,h,w] fp32 0/1, the census maximum taken per sample (the reference runs B = 1).  Every
    step is one correctly rounded fp32 operation, as in torch; the threshold is compared in fp32, as torch compares a float
    tensor with a Python scalar."""
    m = np.asarray(exp_mask, dtype=np.float32)
    one = np.float32(1)
    bare = ((one - (one - m[:, 1]) * (one - m[:, 2])) > np.float32(0.5))[:, None]                  # :129
    d = np.asarray(flow_cam, dtype=np.float32) - np.asarray(flow_fwd, dtype=np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        soft = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])[:, None]                             # :130
        soft = one - soft / soft.max(axis=(1, 2, 3), keepdims=True)                                # :131 (np.max propagates NaN)
        census = soft > np.float32(thresh)                                                         # :132
    bare, census = bare.astype(np.float32), census.astype(np.float32)
    combined = one - (one - bare) * (one - census)                                                 # :134
    return bare, census, combined


def flows(combined, flow_cam, flow_fwd):
    """:136-138 -> flow_fwd_non_rigid, flow_fwd_rigid, total_flow"""
    non_rigid = (np.float32(1) - combined) * flow_fwd
    rigid = combined * flow_cam
    return non_rigid, rigid, rigid + non_rigid


def nearest_index(n_out, n_in):
    """scipy.ndimage.zoom(order=0, mode='constant') along one axis: input index of every output index (-1: cval 0).  The
    coordinate is o * ((n_in - 1) / (n_out - 1)) in double; nearest is floor(c + 0.5); a product that lands beyond the last
    sample (possible at the last index only, by rounding) is outside the input."""
    cc = np.arange(n_out, dtype=np.float64) * (float(n_in - 1) / float(n_out - 1))
    idx = np.floor(cc + 0.5).astype(np.int64)
    idx[cc > n_in - 1] = -1
    return idx


def zoom_nearest(pred, Hg, Wg):
    yi, xi = nearest_index(Hg, pred.shape[0]), nearest_index(Wg, pred.shape[1])
    z = pred[np.maximum(yi, 0)][:, np.maximum(xi, 0)].copy()
    z[yi < 0] = 0
    z[:, xi < 0] = 0
    return z


def mask_counts(obj_map, semantic, pred):
    """mask_error for one mask pred [h,w] -> int64 [6] = tp_0, fp_0, fn_0, tp_1, fp_1, fn_1"""
    label = np.where(np.asarray(semantic) != 26, 255, (np.asarray(obj_map) != 0).astype(np.int64))
    m = zoom_nearest(np.asarray(pred, dtype=np.float32), *label.shape)
    cls = np.where(m >= np.float32(1) - m, 0, 1)                       # argmax of [m, 1 - m]: the first maximum wins
    out = []
    for k in (0, 1):
        gt, res = label == k, (cls == k) & (label != 255)
        out += [np.count_nonzero(gt & res), np.count_nonzero(res & ~gt), np.count_nonzero(~res & gt)]
    return np.array(out, dtype=np.int64)


def png_unfilter(ftype, rows, W, bpp=6):
    """Reconstruct the scanlines byte by byte: Recon(x) = Filt(x) + predictor(a, b, c) mod 256 with a = the byte bpp to the
    left, b = the byte above, c = the byte above a (0 outside the image) -> [H, bpp * W] uint8."""
    H = len(ftype)
    n = bpp * W
    out = np.zeros((H, n), dtype=np.uint8)
    prev = [0] * n
    for y in range(H):
        f = [int(v) for v in rows[y, :n]]
        t = int(ftype[y])
        cur = [0] * n
        for i in range(n):
            a = cur[i - bpp] if i >= bpp else 0
            b = prev[i]
            c = prev[i - bpp] if i >= bpp else 0
            if t == 0:
                p = 0
            elif t == 1:
                p = a
            elif t == 2:
                p = b
            elif t == 3:
                p = (a + b) // 2
            else:
                e = a + b - c
                pa, pb, pc = abs(e - a), abs(e - b), abs(e - c)
                p = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
            cur[i] = (f[i] + p) & 255
        out[y] = cur
        prev = cur
    return out


def flow_from_bytes(recon, W):
    """[H, 6W] reconstructed bytes -> [3,H,W] fp32: the 16-bit samples (most significant byte first), then
    flow_io.py:114-115 `u = (u_.astype('float64') - 2**15) / 64.0` (v likewise), valid as it is, cast by torch.FloatTensor"""
    H = recon.shape[0]
    s = np.ascontiguousarray(recon).view(">u2").reshape(H, W, 3)
    u = (s[..., 0].astype('float64') - 2 ** 15) / 64.0
    v = (s[..., 1].astype('float64') - 2 ** 15) / 64.0
    return np.stack([u, v, s[..., 2].astype('float64')]).astype(np.float32)
