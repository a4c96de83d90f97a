"""Validation metrics on the device (reference loss_functions.py:355-467): thin wrappers over the HIP
entries of cc_amd/csrc/metrics.hip (include/ccengine.h, "validation metrics").

Outputs and workspaces are allocated with torch on the input's device and the kernels never synchronise with the host, so a
validation pass that uses these calls can be captured into a graph.  Results are deterministic run to run (fp64 per-workgroup
partials reduced in a fixed order; exact medians by radix select).
"""
import torch

from ._lib import engine, STREAM

TAU = (3, 0.05)      # outlier_err's default thresholds (loss_functions.py:390)


def _f32(t):
    return t.detach().float().contiguous()


def _mask(m, B):
    """-> (tensor [B,1,Hm,Wm], Hm, Wm, inverted): a mask given as tensor, or as ("1-", tensor) for 1 - tensor without a launch."""
    inv = 0
    if isinstance(m, tuple):
        assert len(m) == 2 and m[0] == "1-", "flow_metrics: a mask is a tensor or ('1-', tensor)"
        inv, m = 1, m[1]
    if m.dim() == 3:
        m = m.unsqueeze(1)
    assert m.dim() == 4 and m.shape[0] == B and m.shape[1] == 1, "flow_metrics: masks must be [B,1,H,W] (got %s)" % (tuple(m.shape),)
    m = _f32(m)
    return m, m.shape[2], m.shape[3], inv


def flow_metrics(gt, rigid_pred, non_rigid_pred=None, masks=(), THRESH=0.5, epe_map=False, tau=TAU):
    """gt [B,Cg,Hg,Wg] (Cg = 2 or 3; channel 2 is the validity mask), predictions [B,2,Hp,Wp], 0-2 rigidity masks [B,1,Hm,Wm] each
    at its own size (or ("1-", mask) for the inverted mask).
    -> 1-D device tensor: [compute_epe, outlier_err] of rigid_pred without a mask (outlier NaN for Cg = 2), else per mask the
    four numbers of compute_all_epes [all_epe, rigid_epe, non_rigid_epe, outliers]; with epe_map=True also the flow_diff map
    [B,Hg,Wg] of the (total, first mask) prediction: (values, map)."""
    B, Cg, Hg, Wg = gt.shape
    assert Cg in (2, 3), "flow_metrics: gt must have 2 or 3 channels"
    assert rigid_pred.dim() == 4 and rigid_pred.shape[:2] == (B, 2), "flow_metrics: predictions must be [B,2,H,W]"
    Hp, Wp = rigid_pred.shape[2:]
    masks = list(masks)
    assert len(masks) <= 2, "flow_metrics: at most two rigidity masks"
    if masks:
        assert non_rigid_pred is not None and non_rigid_pred.shape == rigid_pred.shape, \
            "flow_metrics: masks need non_rigid_pred of the rigid prediction's shape"
        if Cg != 3:
            raise IndexError("flow_metrics: the outlier ratio of compute_all_epes needs the validity channel gt[:, 2]")
    else:
        assert non_rigid_pred is None, "flow_metrics: non_rigid_pred is only used with a rigidity mask"
    dev = gt.device
    g, r = _f32(gt), _f32(rigid_pred)
    nr = _f32(non_rigid_pred) if masks else None
    mk = [_mask(m, B) for m in masks] + [(None, 0, 0, 0)] * (2 - len(masks))
    out = torch.empty(4 * len(masks) if masks else 2, dtype=torch.float32, device=dev)
    emap = torch.empty((B, Hg, Wg), dtype=torch.float32, device=dev) if epe_map else None
    e = engine()
    ws = torch.empty(e.call("cc_flow_metrics_ws", B, Hg, Wg, len(masks)), dtype=torch.uint8, device=dev)
    e.call("cc_flow_metrics", g, Cg, Hg, Wg, r, nr, Hp, Wp, *mk[0], *mk[1], float(THRESH), float(tau[0]), float(tau[1]), B, emap,
           out, ws, STREAM)
    return (out, emap) if epe_map else out


class ErrorSums(object):
    """The running meter of `flow_metrics_samples`: fp64 sums [8] and an int64 count [1] in one 72-byte device buffer, which the
    kernel adds to.  `read()` is the one host read-back -> (sums / count as a list of 8 floats, count)."""

    def __init__(self, device):
        self.buf = torch.zeros(72, dtype=torch.uint8, device=device)
        self.sums, self.count = self.buf[:64].view(torch.float64), self.buf[64:].view(torch.int64)

    def read(self, extra=None):
        """extra: an optional device flag (0-dim bool) that travels with the same copy -> (..., bool(extra))"""
        buf = self.buf if extra is None else torch.cat([self.buf, extra.reshape(1).to(torch.uint8)])
        host = buf.cpu()
        sums, n = host[:64].view(torch.float64), int(host[64:72].view(torch.int64)[0])
        means = [float(v) / n if n else float("nan") for v in sums]
        return (means, n) if extra is None else (means, n, bool(host[72]))


def flow_metrics_samples(flow_pool, obj_pool, table, idx, rigid_pred, non_rigid_pred, mask, max_px, THRESH=0.5, tau=TAU, acc=None):
    """The eight flow errors of validate_flow_with_gt (train.py:748: compute_all_epes with the predicted mask, then with
    1 - obj_map_gt) for B samples whose ground truths differ in size, in one call -> fp32 [B,8] on the device, one row per sample.
    flow_pool / obj_pool: 1-D fp32 device pools; table: device int64 [N,4] rows {flow offset, obj-map offset, Hg, Wg} (offsets in
    floats: the sample's [3,Hg,Wg] (u, v, valid) planes and its [Hg,Wg] object map); idx: device int32 [B], the table rows of
    this batch; rigid_pred / non_rigid_pred [B,2,Hp,Wp]; mask [B,1,Hm,Wm] the predicted rigidity mask; max_px: the largest
    Hg * Wg among the table's rows (the only geometry the host passes).  acc: an `ErrorSums` the rows are added to, in order.
    Row b equals `flow_metrics(gt_b, rigid_pred[b:b+1], non_rigid_pred[b:b+1], masks=(mask[b:b+1], ("1-", obj_b)))` bit for bit."""
    assert flow_pool.dim() == 1 and obj_pool.dim() == 1 and flow_pool.dtype == torch.float32 and obj_pool.dtype == torch.float32, \
        "flow_metrics_samples: the pools are 1-D fp32 tensors"
    assert table.dim() == 2 and table.shape[1] == 4 and table.dtype == torch.int64, "flow_metrics_samples: table must be int64 [N,4]"
    assert idx.dim() == 1 and idx.dtype == torch.int32, "flow_metrics_samples: idx must be int32 [B]"
    B = idx.shape[0]
    assert rigid_pred.dim() == 4 and rigid_pred.shape[:2] == (B, 2) and non_rigid_pred.shape == rigid_pred.shape, \
        "flow_metrics_samples: predictions must be [B,2,H,W] of one shape, B = len(idx)"
    Hp, Wp = rigid_pred.shape[2:]
    m, Hm, Wm, inv = _mask(mask, B)
    assert not inv, "flow_metrics_samples: the predicted mask is not inverted"
    dev = rigid_pred.device
    out = torch.empty((B, 8), dtype=torch.float32, device=dev)
    e = engine()
    ws = torch.empty(e.call("cc_flow_metrics_samples_ws", B, int(max_px)), dtype=torch.uint8, device=dev)
    e.call("cc_flow_metrics_samples", flow_pool, flow_pool.numel(), obj_pool, obj_pool.numel(), table.contiguous(), table.shape[0],
           idx.contiguous(), B, int(max_px), _f32(rigid_pred), _f32(non_rigid_pred), Hp, Wp, m, Hm, Wm, float(THRESH), float(tau[0]),
           float(tau[1]), out, None if acc is None else acc.sums, None if acc is None else acc.count, ws, STREAM)
    return out


def crop_box(H, W, crop=True):
    """Garg / Eigen crop of compute_errors (loss_functions.py:441-444) as rows [y1,y2) x cols [x1,x2); the whole image without."""
    if not crop:
        return 0, H, 0, W
    return int(0.40810811 * H), int(0.99189189 * H), int(0.03594771 * W), int(0.96405229 * W)


def depth_errors(gt, pred, crop=True):
    """compute_errors (loss_functions.py:432-467): gt, pred [B,H,W] -> [6] device tensor [abs_diff, abs_rel, sq_rel, a1, a2, a3]."""
    assert gt.dim() == 3 and pred.shape == gt.shape, "depth_errors: gt and pred must be [B,H,W] of one shape"
    B, H, W = gt.shape
    y1, y2, x1, x2 = crop_box(H, W, crop)
    out = torch.empty(6, dtype=torch.float32, device=gt.device)
    e = engine()
    ws = torch.empty(e.call("cc_depth_errors_ws", B, H, W), dtype=torch.uint8, device=gt.device)
    e.call("cc_depth_errors", _f32(gt), _f32(pred), B, H, W, y1, y2, x1, x2, out, ws, STREAM)
    return out
