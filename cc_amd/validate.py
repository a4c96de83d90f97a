"""Validation loops of the reference's train.py: validate_depth_with_gt (train.py:588-635) and
validate_flow_with_gt (train.py:637-774) on the engine's networks and kernels, same names, argument order and return values
(`errors.avg, error_names`).

What differs from the reference, deliberately:
  * train.py reads a module-global `args`; here the same namespace is passed as `args=` (fields: spatial_normalize, flownet,
    THRESH, and -- only for the optional per-sample hook -- rotation_mode / padding_mode).
  * the ~25 stock-torch launches of the rigidity-mask composition (train.py:673-687) are ONE HIP launch (`cc_rigidity_compose`,
    cc_amd/csrc/validate.hip) -> `rigidity_composition`.
  * the metrics are HIP kernels (cc_amd/metrics.py, cc_amd/csrc/metrics.hip): the eight flow errors of a sample are ONE
    `flow_metrics` call with both rigidity masks, the depth errors one `depth_errors` call (exact medians by radix select, no
    boolean indexing).  No metric call synchronises with the host, so the loop body can be captured into a graph; the values
    stay on the device and are read back once at the end of the loop (`_finish`) instead of eight `.item()` host syncs per
    sample.
  * TensorBoard image / histogram logging and the terminal progress bar (train.py:615-633,700-741,758-768) are UI and out of
    scope; `on_sample(i, dict_of_intermediates)` is the hook a caller's own logging attaches to -- it receives every tensor the
    reference logs.
The reference composes the masks with batch size 1 only (train.py:236: KITTI images differ in size); its broadcasting at
train.py:676 mixes samples for B > 1, so per-sample semantics are what is implemented (identical for B = 1).
"""
import types

import torch

from . import loss_functions as LF
from . import metrics
from ._lib import engine, STREAM
from .inverse_warp import pose2flow
from .logger import AverageMeter

RIGIDITY_FIELDS = ("rigidity_mask", "rigidity_mask_census", "rigidity_mask_combined", "flow_fwd_non_rigid", "flow_fwd_rigid",
                   "total_flow", "oob_rigid", "oob_non_rigid")
DEPTH_ERROR_NAMES = ['abs_diff', 'abs_rel', 'sq_rel', 'a1', 'a2', 'a3']
FLOW_ERROR_NAMES = ['epe_total', 'epe_rigid', 'epe_non_rigid', 'outliers', 'epe_total_with_gt_mask', 'epe_rigid_with_gt_mask',
                    'epe_non_rigid_with_gt_mask', 'outliers_gt_mask']


def rigidity_composition(explainability_mask, flow_cam, flow_fwd, THRESH, want=RIGIDITY_FIELDS):
    """train.py:673-687 in one launch.  explainability_mask [B,MC>=3,H,W], flow_cam / flow_fwd [B,2,H,W] -> namespace with
    rigidity_mask [B,1,H,W], rigidity_mask_census [B,H,W], rigidity_mask_combined [B,1,H,W], flow_fwd_non_rigid, flow_fwd_rigid,
    total_flow [B,2,H,W] (fp32, masks as 0/1) and oob_rigid / oob_non_rigid [B,H,W] (bool, inverse_warp.py:222-238).
    `want`: the fields to produce (the others are None and cost no HBM traffic)."""
    B, MC, H, W = explainability_mask.shape
    assert flow_cam.shape == (B, 2, H, W) and flow_fwd.shape == (B, 2, H, W), "rigidity_composition: flows must be [B,2,H,W] of the mask"
    m = explainability_mask.detach().float().contiguous()
    fc, ff = flow_cam.detach().float().contiguous(), flow_fwd.detach().float().contiguous()
    shapes = dict(rigidity_mask=(B, 1, H, W), rigidity_mask_census=(B, H, W), rigidity_mask_combined=(B, 1, H, W),
                  flow_fwd_non_rigid=(B, 2, H, W), flow_fwd_rigid=(B, 2, H, W), total_flow=(B, 2, H, W),
                  oob_rigid=(B, H, W), oob_non_rigid=(B, H, W))
    unknown = set(want) - set(shapes)
    assert not unknown, "rigidity_composition: unknown fields %s" % sorted(unknown)
    o = {k: (torch.empty(shapes[k], dtype=torch.float32, device=m.device) if k in want else None) for k in RIGIDITY_FIELDS}
    engine().call("cc_rigidity_compose", m, MC, fc, ff, o["rigidity_mask"], o["rigidity_mask_census"], o["rigidity_mask_combined"],
                  o["flow_fwd_non_rigid"], o["flow_fwd_rigid"], o["total_flow"], o["oob_rigid"], o["oob_non_rigid"],
                  float(THRESH), B, H, W, STREAM)
    for k in ("oob_rigid", "oob_non_rigid"):
        if o[k] is not None:
            o[k] = o[k] > 0.5
    return types.SimpleNamespace(**o)


def _device_of(net):
    return next(net.parameters()).device


def _finish(errors):
    """the loop's only host read-back"""
    avg = [a.detach().double() if torch.is_tensor(a) else torch.tensor(float(a), dtype=torch.float64) for a in errors.avg]
    dev = next((a.device for a in avg if a.is_cuda), torch.device("cpu"))
    return torch.stack([a.to(dev) for a in avg]).tolist()


def validate_depth_with_gt(val_loader, disp_net, epoch=0, logger=None, output_writers=(), args=None, on_sample=None):
    """train.py:588-635: Eigen depth errors of disp_net over (tgt_img, depth_gt) batches."""
    error_names = list(DEPTH_ERROR_NAMES)
    errors = AverageMeter(i=len(error_names))
    disp_net.eval()                                                            # :596
    dev = _device_of(disp_net)
    with torch.no_grad():
        for i, (tgt_img, depth) in enumerate(val_loader):
            tgt_img = tgt_img.to(dev)
            output_disp = disp_net(tgt_img)                                    # :602
            if args is not None and getattr(args, "spatial_normalize", False):
                output_disp = LF.spatial_normalize(output_disp)                # :603-604
            output_depth = 1 / output_disp                                     # :606
            depth = depth.to(dev)
            errors.update(list(metrics.depth_errors(depth, output_depth.squeeze(1)).unbind(0)))   # :624 (0-dim device tensors, no sync)
            if on_sample is not None:
                on_sample(i, dict(tgt_img=tgt_img, depth=depth, output_disp=output_disp, output_depth=output_depth))
    return _finish(errors), error_names


def validate_flow_with_gt(val_loader, disp_net, pose_net, mask_net, flow_net, epoch=0, logger=None, output_writers=(),
                          args=None, on_sample=None):
    """train.py:637-774: end-point errors of the composed (rigid + non-rigid) flow against KITTI flow ground truth, once with
    the predicted rigidity mask and once with the ground-truth object map."""
    assert args is not None, "validate_flow_with_gt: pass the training arguments namespace as args= (THRESH, flownet, spatial_normalize)"
    error_names = list(FLOW_ERROR_NAMES)
    errors = AverageMeter(i=len(error_names))
    for net in (disp_net, pose_net, mask_net, flow_net):                      # :644-648
        net.eval()
    dev = _device_of(disp_net)
    nan_seen = None
    with torch.no_grad():
        for i, (tgt_img, ref_imgs, intrinsics, intrinsics_inv, flow_gt, obj_map_gt) in enumerate(val_loader):
            tgt_img = tgt_img.to(dev)
            ref_imgs = [img.to(dev) for img in ref_imgs]
            intrinsics, intrinsics_inv = intrinsics.to(dev), intrinsics_inv.to(dev)
            flow_gt, obj_map_gt = flow_gt.to(dev), obj_map_gt.to(dev)
            disp = disp_net(tgt_img)                                           # :659
            if getattr(args, "spatial_normalize", False):
                disp = LF.spatial_normalize(disp)
            depth = 1 / disp
            pose = pose_net(tgt_img, ref_imgs)
            explainability_mask = mask_net(tgt_img, ref_imgs)
            if getattr(args, "flownet", "Back2Future") == 'Back2Future':       # :666-670
                flow_fwd, flow_bwd, _ = flow_net(tgt_img, ref_imgs[1:3])
            else:
                flow_fwd = flow_net(tgt_img, ref_imgs[2])
                flow_bwd = flow_net(tgt_img, ref_imgs[1])
            flow_cam = pose2flow(depth.squeeze(1), pose[:, 2], intrinsics, intrinsics_inv)       # :672
            r = rigidity_composition(explainability_mask, flow_cam, flow_fwd, args.THRESH,
                                     want=RIGIDITY_FIELDS if on_sample is not None else ("rigidity_mask_combined", "total_flow"))
            bad = torch.isnan(flow_gt.sum()) | torch.isnan(r.total_flow.sum())  # :746 (device flag; reported after the loop)
            nan_seen = bad if nan_seen is None else (nan_seen | bad)
            # :748, both compute_all_epes calls in one: the predicted mask and 1 - obj_map_gt (:689, inverted in the kernel)
            _epe_errors = list(metrics.flow_metrics(flow_gt, flow_cam, flow_fwd, masks=(r.rigidity_mask_combined, ("1-", obj_map_gt)),
                                                    THRESH=0.5).unbind(0))
            errors.update(_epe_errors)
            if on_sample is not None:
                on_sample(i, dict(tgt_img=tgt_img, ref_imgs=ref_imgs, flow_gt=flow_gt, depth=depth, pose=pose,
                                  explainability_mask=explainability_mask, flow_fwd=flow_fwd, flow_bwd=flow_bwd, flow_cam=flow_cam,
                                  epe_errors=_epe_errors, **vars(r)))
    if nan_seen is not None and bool(nan_seen):
        print('NaN encountered')                                               # :747
    return _finish(errors), error_names


# ------------------------------------------------------------------------------------- the same two passes over resident stores
def validate_flow_from_store(store, disp_net, pose_net, mask_net, flow_net, batch_size=1, args=None, on_batch=None):
    """validate_flow_with_gt over a `datasets.FlowValStore`, batch_size samples at a time -> (errors, error_names).  Per batch: the
    four forward passes, pose2flow, the per-sample composition and ONE `metrics.flow_metrics_samples` call, which scores every
    sample against its own ground truth (read where it lies, through the store's table) and adds the rows to a device meter in
    sample order.  The NaN flag of train.py:746 stays on the device; the meter and the flag are read back once, after the loop;
    errors = sums / count in fp64 (the sums are fp64 where AverageMeter's are fp32).  At batch_size=1 every row is what
    validate_flow_with_gt computes for that sample; larger batches change only what the networks' own kernels make of a batch.
    on_batch(k, dict): the hook of a caller's own logging, called per batch with idx, the rows [b,8] and the tensors they were
    computed from (flow_cam, flow_fwd, rigidity_mask_combined, total_flow)."""
    from .datasets import DeviceFlowValLoader
    assert args is not None, "validate_flow_from_store: pass the training arguments namespace as args= (THRESH, flownet, spatial_normalize)"
    for net in (disp_net, pose_net, mask_net, flow_net):
        net.eval()
    acc = metrics.ErrorSums(store.device)
    nan_seen = store.gt_nan()
    with torch.no_grad():
        for k, (tgt_img, ref_imgs, intrinsics, intrinsics_inv, idx) in enumerate(DeviceFlowValLoader(store, batch_size).batches()):
            flow_cam, flow_fwd, r = _flow_batch(tgt_img, ref_imgs, intrinsics, intrinsics_inv, disp_net, pose_net, mask_net, flow_net, args)
            nan_seen = nan_seen | torch.isnan(r.total_flow.sum())
            rows = metrics.flow_metrics_samples(store.flow_pool, store.obj_pool, store.table, idx, flow_cam, flow_fwd,
                                                r.rigidity_mask_combined, store.max_px, THRESH=0.5, acc=acc)
            if on_batch is not None:
                on_batch(k, dict(idx=idx, rows=rows, flow_cam=flow_cam, flow_fwd=flow_fwd, rigidity_mask_combined=r.rigidity_mask_combined,
                                 total_flow=r.total_flow))
    errors, _, nan = acc.read(extra=nan_seen)                                  # the loop's only host read-back
    if nan:
        print('NaN encountered')
    return errors, list(FLOW_ERROR_NAMES)


def _flow_batch(tgt_img, ref_imgs, intrinsics, intrinsics_inv, disp_net, pose_net, mask_net, flow_net, args):
    """train.py:659-687 for one batch -> (flow_cam, flow_fwd, composition)"""
    disp = disp_net(tgt_img)
    if getattr(args, "spatial_normalize", False):
        disp = LF.spatial_normalize(disp)
    depth = 1 / disp
    pose = pose_net(tgt_img, ref_imgs)
    explainability_mask = mask_net(tgt_img, ref_imgs)
    if getattr(args, "flownet", "Back2Future") == 'Back2Future':
        flow_fwd, _, _ = flow_net(tgt_img, ref_imgs[1:3])
    else:
        flow_fwd = flow_net(tgt_img, ref_imgs[2])
    flow_cam = pose2flow(depth.squeeze(1), pose[:, 2], intrinsics, intrinsics_inv)
    r = rigidity_composition(explainability_mask, flow_cam, flow_fwd, args.THRESH, want=("rigidity_mask_combined", "total_flow"))
    return flow_cam, flow_fwd, r


def validate_without_gt_from_store(store, disp_net, pose_net, mask_net, flow_net, batch_size, cfg, normalize="global"):
    """The validation signal that needs no labels: the training losses (train.py:490-509) of the four networks in eval() mode over a
    `datasets.FrameStore` built with train=False -- the `SequenceFolder(train=False)` train.py:209-215 builds "to measure photometric
    loss from warping" and no reference validator ever reads.  -> (values, names), names = ledger.LOSS_NAMES: the total and the five
    terms, each the mean over the store's samples.
    Batches: the samples in the store's (val.txt) order, not augmented -- ArrayToTensor + Normalize (train.py:187; normalize='local':
    NormalizeLocally), frames read where they lie; every sample is scored, the last batch may be short and weighs by its size.
    Per batch `trainer.cc_forward` under torch.no_grad(): the eval-mode outputs are one full-resolution level each, so every term
    is its single-scale, forward-only form (no gradient is computed or stashed).  cfg: a trainer.StepConfig (weights, wssim, qch,
    THRESH, smoothness_type, spatial_normalize, no_non_rigid_mask ..).  The values are folded into fp64 on the device by a Ledger of
    this call's own and read back once, after the loop."""
    import numpy as np
    from .custom_transforms import DeviceTrainTransform
    from .ledger import Ledger, LOSS_NAMES
    from .step_scope import StepScope
    from .trainer import cc_forward
    if batch_size < 1 or len(store) < 1:
        raise ValueError("validate_without_gt_from_store: batch size %d over %d samples" % (batch_size, len(store)))
    nets = (disp_net, pose_net, mask_net, flow_net)
    for net in nets:
        net.eval()
    dev = store.device
    prep = DeviceTrainTransform(device=dev, normalize=normalize)          # (its frame converter and local normalisation; no draws)
    meter = Ledger(dev, capacity=64)
    S, nf = store.samples.shape
    _, H, W, _ = store.frames.shape
    one = 3 * H * W
    with torch.no_grad():
        for lo in range(0, S, batch_size):
            ids = np.arange(lo, min(S, lo + batch_size))
            b = ids.size
            x = prep.frames.store_to_tensor(store, store.samples_np[ids].T.reshape(-1)).view(nf, b, 3, H, W)    # frame-major
            if prep.local:
                prep._local_norm(x, b, nf, one, b * one)
            K = store.intrinsics_np[store.sample_scene_np[ids]]
            KK = torch.from_numpy(np.stack([K, np.stack([np.linalg.inv(k) for k in K])])).to(dev)
            flags = []
            with StepScope(nan_flags=flags):
                out = cc_forward(nets, (x[0], [x[j] for j in range(1, nf)], KK[0], KK[1]), cfg)
            LF.pyramid_cache.clear()
            LF.take_nan_flags()                                            # (they are sources of the meter's row instead)
            meter.append({k: (v.reshape(1) if torch.is_tensor(v) else v) for k, v in out.items()}, b, nan_flags=flags)
    avg = meter.average()                                                  # the loop's only host read-back
    if avg["nan"]["avg"] > 0:
        print('NaN encountered')
    return [avg[k]["avg"] for k in LOSS_NAMES], list(LOSS_NAMES)


def validate_depth_from_store(store, disp_net, batch_size, args=None):
    """validate_depth_with_gt over a `datasets.DepthValStore` -> (errors, error_names).  As there, every batch's mean counts once
    (AverageMeter.update(n=1), so a short last batch weighs as much as a full one); the six errors are summed in fp64 on the
    device and read back once."""
    from .datasets import DeviceDepthValLoader
    disp_net.eval()
    total, n = torch.zeros(len(DEPTH_ERROR_NAMES), dtype=torch.float64, device=store.device), 0
    with torch.no_grad():
        for tgt_img, depth in DeviceDepthValLoader(store, batch_size):
            output_disp = disp_net(tgt_img)
            if args is not None and getattr(args, "spatial_normalize", False):
                output_disp = LF.spatial_normalize(output_disp)
            total += metrics.depth_errors(depth, (1 / output_disp).squeeze(1)).double()
            n += 1
    return (total / n).tolist(), list(DEPTH_ERROR_NAMES)
