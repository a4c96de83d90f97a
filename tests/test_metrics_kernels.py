"""Validation-metric kernels (cc_amd/csrc/metrics.hip through cc_amd/metrics.py; reference loss_functions.py:355-467).

CPU: the same kernel sources on x86 (tests/hipemu) against the reference-written fixtures (tests/golden/metrics.npz) and against
the CPU path of cc_amd.loss_functions (the reference's expressions on ATen).  GPU: the public loss_functions on HIP tensors against
the fixtures and against oracle/metrics.py at KITTI sizes, and a graph capture of the metrics (no host sync inside)."""
import os

import numpy as np
import pytest
import torch

from cc_amd import loss_functions as LF
from cc_amd import metrics as M
from oracle import metrics as OM
from oracle.make_golden import metric_inputs


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "metrics.npz"))


@pytest.fixture
def emu():
    from hipemu.emu import emulated_engine
    with emulated_engine() as e:
        yield e


def _close(a, b, tol):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.max(np.abs(a - b)) <= tol * max(1.0, np.max(np.abs(b))), (a, b)


def _rel(a, b, tol):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert np.all(np.abs(a - b) <= tol * np.maximum(np.abs(b), 1e-12)), (a, b)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _seeded(seed):
    return np.random.RandomState(seed)


# ------------------------------------------------------------------------------------------------------------------ CPU (emulator)
def test_metrics_golden_emulated(emu, gold):
    m = metric_inputs()
    out, emap = M.flow_metrics(m["gt"], m["rigid"], epe_map=True)
    _close(emap.numpy(), gold["flow_diff"], 1e-6)
    _close(out[0], gold["epe3"], 1e-6)
    _close(out[1], gold["outlier"], 1e-6)
    _close(M.flow_metrics(m["gt"][:, :2].contiguous(), m["nonrigid"])[0], gold["epe2"], 1e-6)
    _close(M.flow_metrics(m["gt"], m["rigid"], m["nonrigid"], masks=(m["mask"],)).numpy(), gold["all_epes"], 1e-6)
    _close(M.depth_errors(m["dgt"], m["dpred"]).numpy(), gold["errors_crop"], 1e-6)
    _close(M.depth_errors(m["dgt"], m["dpred"], crop=False).numpy(), gold["errors_nocrop"], 1e-6)


def _flow_case(B, Hg, Wg, Hp, Wp, mask_hw, seed, valid_frac=0.7):
    r = _seeded(seed)
    gt = np.concatenate([r.randn(B, 2, Hg, Wg) * 6.0, (r.rand(B, 1, Hg, Wg) < valid_frac)], 1).astype(np.float32)
    rigid = (r.randn(B, 2, Hp, Wp) * 3.0).astype(np.float32)
    nonrigid = (r.randn(B, 2, Hp, Wp) * 3.0).astype(np.float32)
    masks = [r.rand(B, 1, h, w).astype(np.float32) for h, w in mask_hw]
    t = torch.from_numpy
    return t(gt), t(rigid), t(nonrigid), [t(m) for m in masks]


def _check_all_epes(got, gt, want, tol):
    """sums to `tol` relative; the outlier ratio to one pixel (ulp-level interpolation can move a pixel across a threshold)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    _rel(got[:3], want[:3], tol)
    nvalid = float(gt[:, 2].double().sum())
    assert abs(got[3] - want[3]) * nvalid <= 1.0 + 1e-3, (got[3], want[3], nvalid)


@pytest.mark.parametrize("B", [1, 3])
def test_flow_metrics_shapes_emulated(emu, B):
    # KITTI's 375x1242 -> 256x832 in miniature (non-integer ratios), one mask at the prediction size and one at the gt size
    Hg, Wg, Hp, Wp = 47, 155, 32, 104
    gt, rigid, nonrigid, masks = _flow_case(B, Hg, Wg, Hp, Wp, [(Hp, Wp), (Hg, Wg)], seed=5 + B)
    got = M.flow_metrics(gt, rigid, nonrigid, masks=masks, THRESH=0.5).numpy()
    for k, m in enumerate(masks):
        want = LF.compute_all_epes(gt, rigid, nonrigid, m, THRESH=0.5)
        _check_all_epes(got[4 * k:4 * k + 4], gt, want, 1e-6)
    # the inverted mask of validate_flow_with_gt (1 - obj_map without a launch)
    inv = M.flow_metrics(gt, rigid, nonrigid, masks=(("1-", masks[1]),)).numpy()
    _check_all_epes(inv, gt, LF.compute_all_epes(gt, rigid, nonrigid, 1 - masks[1]), 1e-6)
    # no mask: compute_epe / outlier_err / flow_diff, 3- and 2-channel ground truth
    out, emap = M.flow_metrics(gt, rigid, epe_map=True)
    _rel(out[0], LF.compute_epe(gt, rigid), 1e-6)
    want_out = LF.outlier_err(gt, rigid)
    assert abs(float(out[1]) - want_out) * float(gt[:, 2].sum()) <= 1.0 + 1e-3
    # per pixel: the kernels follow upsample_bilinear2d's fp32 source index (the HIP ATen kernel); CPU ATen forms the index in
    # fp64, so at non-integer ratios its weights differ by up to 1 fp32 ulp of the source coordinate (~4e-6 here)
    ref_map = LF.flow_diff(gt, rigid)
    assert np.allclose(emap.numpy(), ref_map.numpy(), rtol=1e-5, atol=2e-4)
    gt2 = gt[:, :2].contiguous()
    out2, emap2 = M.flow_metrics(gt2, nonrigid, epe_map=True)
    _rel(out2[0], LF.compute_epe(gt2, nonrigid), 1e-6)
    assert np.isnan(float(out2[1]))
    assert np.allclose(emap2.numpy(), LF.flow_diff(gt2, nonrigid).numpy(), rtol=1e-5, atol=2e-4)
    with pytest.raises(IndexError):                      # compute_all_epes' outlier ratio needs gt[:, 2], as the reference
        M.flow_metrics(gt2, rigid, nonrigid, masks=masks[:1])


def _depth_case():
    """five samples of 24x40: odd / even valid counts with heavy duplicates, one valid pixel, no valid pixel, a NaN prediction"""
    r = _seeded(3)
    B, H, W = 5, 24, 40
    gt = (r.rand(B, H, W) * 100.0 - 10.0).astype(np.float32)
    pred = (r.rand(B, H, W) * 60.0 + 0.5).astype(np.float32)
    gt[0] = np.round(gt[0] / 10.0) * 10.0 + 0.5                 # few distinct values
    pred[0] = np.round(pred[0] / 7.0) * 7.0
    pred[0, 0, :5] = -3.0                                      # clamped to 1e-3
    pred[1, 3, :7] = 200.0                                     # clamped to 80
    gt[2] = 0.0
    gt[2, 15, 20] = 12.5                                       # one valid pixel (inside the crop box)
    gt[3] = 90.0                                               # no valid pixel
    pred[4, 18, 10] = np.nan                                   # NaN among the valid predictions
    t = torch.from_numpy
    return t(gt), t(pred)


def _valid_count(g, crop):
    y1, y2, x1, x2 = M.crop_box(g.shape[0], g.shape[1], crop)
    ok = (g > 0) & (g < 80)
    return int(ok[y1:y2, x1:x2].sum())


def _check_depth(got, want):
    got = np.asarray(got, dtype=np.float32)
    want = np.asarray([float(v) for v in want], dtype=np.float32)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    ok = ~np.isnan(want)
    assert np.array_equal(got[3:][ok[3:]], want[3:][ok[3:]]), (got, want)          # a1..a3: exact counts
    _rel(got[:3][ok[:3]], want[:3][ok[:3]], 1e-6)


@pytest.mark.parametrize("crop", [True, False])
def test_depth_errors_edges_emulated(emu, crop):
    gt, pred = _depth_case()
    counts = [_valid_count(g, crop) for g in gt]
    assert counts[2] == 1 and counts[3] == 0
    for b in range(gt.shape[0]):
        _check_depth(M.depth_errors(gt[b:b + 1], pred[b:b + 1], crop).numpy(), LF.compute_errors(gt[b:b + 1], pred[b:b + 1], crop))
    if crop:
        assert counts[0] % 2 != counts[1] % 2 or counts[0] != counts[1]
    # several samples in one call: summed in sample order, / B
    _check_depth(M.depth_errors(gt[:3], pred[:3], crop).numpy(), LF.compute_errors(gt[:3], pred[:3], crop))
    _check_depth(M.depth_errors(gt, pred, crop).numpy(), LF.compute_errors(gt, pred, crop))


def test_depth_median_parity_emulated(emu):
    # odd and even valid counts: the lower median (torch.median) decides the scale, so the exact counts a1..a3 pin it
    r = _seeded(11)
    for n_valid in (7, 8, 33, 64):
        gt = np.full((1, 8, 8), 95.0, dtype=np.float32)
        pred = np.ones((1, 8, 8), dtype=np.float32)
        idx = r.permutation(64)[:n_valid]
        gt.reshape(-1)[idx] = (r.randint(1, 6, n_valid) * 3.0).astype(np.float32)       # heavy duplicates
        pred.reshape(-1)[idx] = (r.rand(n_valid) * 20.0 + 0.1).astype(np.float32)
        g, p = torch.from_numpy(gt), torch.from_numpy(pred)
        _check_depth(M.depth_errors(g, p, crop=False).numpy(), LF.compute_errors(g, p, crop=False))


def test_metrics_deterministic_emulated(emu):
    gt, rigid, nonrigid, masks = _flow_case(2, 47, 155, 32, 104, [(32, 104), (47, 155)], seed=9)
    a = M.flow_metrics(gt, rigid, nonrigid, masks=masks)
    b = M.flow_metrics(gt, rigid, nonrigid, masks=masks)
    assert _same_bits(a, b)
    dg, dp = _depth_case()
    assert _same_bits(M.depth_errors(dg, dp), M.depth_errors(dg, dp))
    assert _same_bits(M.depth_errors(dg[:3], dp[:3], crop=False), M.depth_errors(dg[:3], dp[:3], crop=False))


# ------------------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_metrics_golden_through_loss_functions_gpu(gold):
    m = {k: v.cuda() for k, v in metric_inputs().items()}
    _close(LF.flow_diff(m["gt"], m["rigid"]).cpu().numpy(), gold["flow_diff"], 2e-5)
    _close(LF.compute_epe(m["gt"], m["rigid"]), gold["epe3"], 2e-5)
    _close(LF.compute_epe(m["gt"][:, :2].contiguous(), m["nonrigid"]), gold["epe2"], 2e-5)
    _close(LF.outlier_err(m["gt"], m["rigid"]), gold["outlier"], 2e-5)
    _close(LF.compute_all_epes(m["gt"], m["rigid"], m["nonrigid"], m["mask"]), gold["all_epes"], 2e-5)
    _close([float(v) for v in LF.compute_errors(m["dgt"], m["dpred"])], gold["errors_crop"], 2e-5)
    _close([float(v) for v in LF.compute_errors(m["dgt"], m["dpred"], crop=False)], gold["errors_nocrop"], 2e-5)
    out = LF.compute_all_epes(m["gt"], m["rigid"], m["nonrigid"], m["mask"], sync=False)
    assert all(torch.is_tensor(v) and v.dim() == 0 and v.is_cuda for v in out)


@pytest.mark.gpu
def test_metrics_kitti_sizes_gpu():
    gt, rigid, nonrigid, masks = _flow_case(1, 375, 1242, 256, 832, [(256, 832), (375, 1242)], seed=17, valid_frac=0.3)
    got = M.flow_metrics(gt.cuda(), rigid.cuda(), nonrigid.cuda(), masks=[m.cuda() for m in masks]).cpu().numpy()
    for k, m in enumerate(masks):
        _check_all_epes(got[4 * k:4 * k + 4], gt, OM.compute_all_epes(gt, rigid, nonrigid, m), 1e-5)
    r = _seeded(19)
    dgt = torch.from_numpy((r.rand(2, 375, 1242) * 100.0 - 10.0).astype(np.float32))
    dpred = torch.from_numpy((r.rand(2, 375, 1242) * 60.0 + 0.5).astype(np.float32))
    got = M.depth_errors(dgt.cuda(), dpred.cuda()).cpu().numpy()
    want = np.asarray(OM.compute_errors(dgt, dpred), dtype=np.float64)
    assert np.array_equal(got[3:], want[3:].astype(np.float32)), (got, want)
    _rel(got[:3], want[:3], 1e-5)


@pytest.mark.gpu
def test_metrics_graph_capture_gpu():
    dev = torch.device("cuda")
    gt, rigid, nonrigid, masks = _flow_case(1, 47, 155, 32, 104, [(32, 104)], seed=23)
    dg, dp = _depth_case()
    dg, dp = dg[:2].contiguous(), dp[:2].contiguous()
    static = [t.to(dev) for t in (gt, rigid, nonrigid, masks[0], dg, dp)]

    def run(s_gt, s_r, s_nr, s_m, s_dg, s_dp):
        return torch.stack(LF.compute_errors(s_dg, s_dp) + LF.compute_all_epes(s_gt, s_r, s_nr, s_m, sync=False))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(*static)                                       # warm-up off the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run(*static)
    # new inputs into the static buffers, replay, compare with an eager call bit for bit
    gt2, rigid2, nonrigid2, masks2 = _flow_case(1, 47, 155, 32, 104, [(32, 104)], seed=29)
    r = _seeded(31)
    dg2 = torch.from_numpy((r.rand(*dg.shape) * 100.0 - 10.0).astype(np.float32))
    dp2 = torch.from_numpy((r.rand(*dp.shape) * 60.0 + 0.5).astype(np.float32))
    for s, t in zip(static, (gt2, rigid2, nonrigid2, masks2[0], dg2, dp2)):
        s.copy_(t)
    graph.replay()
    eager = run(*[t.to(dev) for t in (gt2, rigid2, nonrigid2, masks2[0], dg2, dp2)])
    eager2 = run(*[t.to(dev) for t in (gt2, rigid2, nonrigid2, masks2[0], dg2, dp2)])
    torch.cuda.synchronize()
    assert _same_bits(eager, eager2)
    assert _same_bits(captured, eager), (captured, eager)
