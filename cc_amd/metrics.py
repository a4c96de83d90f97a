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
