"""KITTI evaluation (cc_amd/csrc/kitti_eval.hip through cc_amd/kitti_eval.py; reference kitti_eval/, test_disp.py, test_pose.py).

CPU: the kernel sources on x86 (tests/hipemu) and the NumPy restatement tests/kitti_eval_np.py against the reference-written
fixture tests/golden/kitti_eval.npz (tools/make_kitti_eval_golden.py), the readers on tiny synthetic KITTI trees.  GPU: the four
entries at KITTI sizes against the restatement, run-to-run bit equality, a graph capture of one sample's depth evaluation, and
both evaluation loops end to end with randomly initialised networks."""
import datetime
import os
import pathlib

import numpy as np
import pytest
import torch

import kitti_eval_cases as C
import kitti_eval_np as R
from cc_amd import kitti_eval as K


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "kitti_eval.npz"))


@pytest.fixture
def emu():
    from hipemu.emu import emulated_engine
    with emulated_engine() as e:
        yield e


def _dense(gold, name, H, W):
    d = np.zeros(H * W, dtype=np.float32)
    d[gold["velo_%s_idx" % name]] = gold["velo_%s_val" % name]
    return d.reshape(H, W)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _rel(a, b, tol):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.all(np.abs(a - b) <= tol * np.maximum(np.abs(b), 1e-12)), (a, b)


def _check_eigen(got, want, n_valid, tol=1e-5):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    _rel(got[:, :4], want[:, :4], tol)
    assert np.all(np.abs(got[:, 4:] - want[:, 4:]) <= 2.0 / n_valid + 1e-12), (got, want)


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t if dtype is None else t.to(dtype)


# ----------------------------------------------------------------------------------------------------- fixture sanity (CPU)
def test_cases_plant_the_edge_cases():
    H, W = 24, 40
    P = C.P_velo2im(W, H)
    pts = C.velo_points(H, W, 300, 1).astype(np.float64)
    pts[:, 3] = 1
    pr = pts @ P.T
    keep = pts[:, 0] >= 0
    u, v = pr[keep, 0] / pr[keep, 2], pr[keep, 1] / pr[keep, 2]
    assert np.any(np.abs(u - np.floor(u) - 0.5) == 0) and np.any(np.abs(v - np.floor(v) - 0.5) == 0)   # exact ties
    assert np.any(pr[keep, 2] < 0)                                                                        # negative z
    assert np.any(~keep)                                                                                  # x < 0
    ui, vi = np.round(u) - 1, np.round(v) - 1
    ok = (ui >= 0) & (vi >= 0) & (ui < W) & (vi < H)
    assert np.any(~ok)                                                                                     # out of bounds
    pix = (vi * W + ui)[ok]
    assert len(np.unique(pix)) < len(pix)                                                                 # duplicates
    assert np.any((ui[ok] == W - 1)) and np.any(ui[ok] == 0)                                              # collisions


# ------------------------------------------------------------------------------------------- restatement vs fixture (CPU)
@pytest.mark.parametrize("case", C.VELO_CASES, ids=[c[0] for c in C.VELO_CASES])
def test_velo_depth_restatement_matches_reference(gold, case):
    name, H, W, n, seed = case
    got = R.velo_depth(C.velo_points(H, W, n, seed), C.P_velo2im(W, H), H, W)
    assert _same_bits(got, _dense(gold, name, H, W))


def _zoom_check(got, gold, name, H, W):
    if name in gold:
        assert _same_bits(got, gold[name])
    else:
        rows, cols = C.zoom_keep(H, W)
        assert _same_bits(got[rows], gold[name + "_rows"])
        assert _same_bits(np.ascontiguousarray(got[:, cols]), gold[name + "_cols"])


@pytest.mark.parametrize("case", C.ZOOM_CASES, ids=[c[0] for c in C.ZOOM_CASES])
def test_spline_zoom_restatement_matches_reference(gold, case):
    name, h, w, H, W, seed = case
    _zoom_check(R.spline_zoom(C.zoom_source(h, w, seed), H, W, 1e-3, 80), gold, name, H, W)


def test_eigen_and_pose_restatement_match_reference(gold):
    for name, even, seed in (("e_even", True, 14), ("e_odd", False, 15)):
        gt, pred, disp, norm = C.eigen_case(seed, even=even)
        n = int(((gt > 1e-3) & (gt < 80) & R.crop_mask(*gt.shape)).sum())
        _check_eigen(R.eigen_errors(gt, pred, 1e-3, 80, disp, norm), gold[name], n, 1e-9)
    for name, L, mode, S, seed in C.POSE_CASES:
        pred, seq, first = C.pose_case(L, S, seed)
        err, fin = R.pose_snippet_errors(pred, seq, first, mode)
        _rel(err, gold[name + "_err"], 1e-6)
        assert np.allclose(fin, gold[name + "_final"], rtol=1e-6, atol=1e-6)


# -------------------------------------------------------------------------------------------------- kernels, emulated (CPU)
def test_velo_depth_emulated(emu, gold):
    for name, H, W, n, seed in C.VELO_CASES:
        got = K.velo_depth(_t(C.velo_points(H, W, n, seed)), _t(C.P_velo2im(W, H)), H, W).numpy()
        assert _same_bits(got, _dense(gold, name, H, W)), name


@pytest.mark.parametrize("case", [c for c in C.ZOOM_CASES if c[0] in ("z_small", "z_mid", "z_1241")],
                         ids=lambda c: c[0])
def test_spline_zoom_emulated(emu, gold, case):
    name, h, w, H, W, seed = case
    got = K.spline_zoom(_t(C.zoom_source(h, w, seed)), H, W, 1e-3, 80).numpy()
    _zoom_check(got, gold, name, H, W)
    if H == 376:
        assert np.all(got[-1] == np.float32(1e-3))          # 375 * (255/375) > 255: cval 0 for the whole row, clipped
    # a batch of two images equals two single calls
    src2 = np.stack([C.zoom_source(h, w, seed), C.zoom_source(h, w, seed + 100)])
    both = K.spline_zoom(_t(src2), H, W, 1e-3, 80).numpy()
    assert _same_bits(both[0], got)


def test_eigen_errors_emulated(emu, gold):
    for name, even, seed in (("e_even", True, 14), ("e_odd", False, 15)):
        gt, pred, disp, norm = C.eigen_case(seed, even=even)
        n = int(((gt > 1e-3) & (gt < 80) & R.crop_mask(*gt.shape)).sum())
        got = K.eigen_errors(_t(gt), _t(pred), 1e-3, 80, _t(disp), _t(norm)).numpy()
        _check_eigen(got, gold[name], n)
        plain = K.eigen_errors(_t(gt), _t(pred), 1e-3, 80).numpy()
        assert np.all(plain[0] == 0) and _same_bits(plain[1], got[1])
    # median pair: an even count takes the mean of the two middle values (np.median), not the lower one (torch.median)
    gt = np.zeros((10, 10), np.float32)
    pred = np.ones((10, 10), np.float32)
    gt[6:8, 2:4] = [[2.0, 4.0], [6.0, 8.0]]
    pred[6:8, 2:4] = [[1.0, 1.0], [3.0, 3.0]]
    got = K.eigen_errors(_t(gt), _t(pred)).numpy()
    _check_eigen(got, R.eigen_errors(gt, pred), 4, 1e-12)


def test_velo_to_eigen_chain_emulated(emu, gold):
    name, H, W, n, seed = C.VELO_CASES[0]
    gt = K.velo_depth(_t(C.velo_points(H, W, n, seed)), _t(C.P_velo2im(W, H)), H, W).numpy()
    mask = (gt.astype(np.float64) > 1e-3) & (gt < 80) & R.crop_mask(H, W)
    assert np.array_equal(np.flatnonzero(mask), gold["velo_%s_mask" % name])


@pytest.mark.parametrize("case", C.POSE_CASES, ids=[c[0] for c in C.POSE_CASES])
def test_pose_snippet_errors_emulated(emu, gold, case):
    name, L, mode, S, seed = case
    pred, seq, first = C.pose_case(L, S, seed)
    err, fin = K.pose_snippet_errors(_t(pred), _t(seq), _t(first), mode, want_final=True)
    _rel(err.numpy(), gold[name + "_err"], 1e-6)
    assert np.allclose(fin.numpy(), gold[name + "_final"], rtol=1e-6, atol=1e-6)


def test_kernels_deterministic_emulated(emu):
    H, W = 24, 40
    pts, P = _t(C.velo_points(H, W, 300, 1)), _t(C.P_velo2im(W, H))
    assert _same_bits(K.velo_depth(pts, P, H, W).numpy(), K.velo_depth(pts, P, H, W).numpy())
    gt, pred, disp, norm = C.eigen_case(14)
    a = K.eigen_errors(_t(gt), _t(pred), 1e-3, 80, _t(disp), _t(norm)).numpy()
    b = K.eigen_errors(_t(gt), _t(pred), 1e-3, 80, _t(disp), _t(norm)).numpy()
    assert _same_bits(a, b)


# ------------------------------------------------------------------------------------------------------ readers (CPU)
def _png(path, arr):
    from PIL import Image
    path.parent.mkdir(parents=True, exist_ok=True)
    Image.fromarray(arr).save(str(path))


def make_raw_tree(root, H=24, W=40, frames=4, seed=0):
    """a tiny KITTI raw drive: date/scene with image_02 PNGs, velodyne .bin, oxts, and the date's calib files -> test list"""
    r = np.random.RandomState(seed)
    date, scene = "2011_09_26", "2011_09_26_drive_0002_sync"
    d = root / date
    d.mkdir(parents=True)
    cam2cam, velo2cam = C.calib(W, H)
    fmt = lambda a: " ".join(repr(float(x)) for x in a)          # noqa: E731
    (d / "calib_cam_to_cam.txt").write_text("calib_time: 09-Jan-2012 13:57:47\n" +
                                            "".join("%s: %s\n" % (k, fmt(v)) for k, v in cam2cam.items()))
    (d / "calib_velo_to_cam.txt").write_text("calib_time: 15-Mar-2012 11:37:16\nR: %s\nT: %s\n" % (fmt(velo2cam["R"]),
                                                                                                fmt(velo2cam["T"])))
    s = d / scene
    t0 = datetime.datetime(2011, 9, 26, 13, 2, 25)
    stamps = []
    for i in range(frames):
        _png(s / "image_02" / "data" / ("%010d.png" % i), (r.rand(H, W, 3) * 255).astype(np.uint8))
        (s / "velodyne_points" / "data").mkdir(parents=True, exist_ok=True)
        C.velo_points(H, W, 200, seed + i).tofile(str(s / "velodyne_points" / "data" / ("%010d.bin" % i)))
        (s / "oxts" / "data").mkdir(parents=True, exist_ok=True)
        vals = np.zeros(30)
        vals[8:11] = [3.0 + i, 4.0, 0.0]
        (s / "oxts" / "data" / ("%010d.txt" % i)).write_text(" ".join("%.6f" % x for x in vals) + "\n")
        stamps.append((t0 + datetime.timedelta(seconds=0.1 * i + 0.0123)).strftime("%Y-%m-%d %H:%M:%S.%f") + "123")
    (s / "oxts" / "timestamps.txt").write_text("\n".join(stamps) + "\n")
    return ["%s/%s/image_02/data/%010d.png" % (date, scene, i) for i in (0, 2)], (H, W)


def make_odometry_tree(root, H=24, W=40, frames=(6, 5), seed=0):
    r = np.random.RandomState(seed)
    (root / "poses").mkdir(parents=True)
    for k, F in enumerate(frames):
        name = "%02d" % (9 + k)
        for i in range(F):
            _png(root / "sequences" / name / "image_2" / ("%06d.png" % i), (r.rand(H, W, 3) * 255).astype(np.uint8))
        _, seq, _ = C.pose_case(3, 1, seed + k)
        seq = seq[:F] if len(seq) >= F else np.concatenate([seq] * F)[:F]
        np.savetxt(str(root / "poses" / ("%s.txt" % name)), seq.reshape(F, 12), fmt="%.12e")
    return ["09", "1*"]


def test_raw_reader(tmp_path):
    files, (H, W) = make_raw_tree(tmp_path)
    fw = K.KittiRawEigen(tmp_path, files, seq_length=3)
    assert len(fw) == 2
    s0 = fw[0]
    assert s0["tgt"].dtype == np.uint8 and s0["tgt"].shape == (H, W, 3)
    assert len(s0["ref"]) == 2
    # frame 0 has no frame -1: the target stands in, shift 0 -> displacement 0 (read_scene_data :84-89)
    assert np.array_equal(s0["ref"][0], s0["tgt"]) and s0["displacements"][0] == 0
    assert abs(s0["displacements"][1] - 5.0 * 0.1) < 1e-6                     # |v| = 5 m/s, 0.1 s
    s1 = fw[1]
    assert abs(s1["displacements"][0] - np.hypot(5.0, 4.0) * 0.1) < 1e-6
    assert np.array_equal(s1["velo"], C.velo_points(H, W, 200, 2))
    assert np.array_equal(s1["P_velo2im"], C.P_velo2im(W, H))
    assert len(K.KittiRawEigen(tmp_path, files, seq_length=0)[0]["ref"]) == 0


def test_odometry_reader(tmp_path):
    make_odometry_tree(tmp_path)
    fw = K.KittiOdometry(tmp_path, ["09", "1*"], seq_length=3)
    assert [s["name"] for s in fw.sequences] == ["09", "10"]
    assert fw.n_frames == 11 and len(fw) == (6 - 2) + (5 - 2)
    assert list(fw.sequences[0]["first"]) == [0, 1, 2, 3]
    assert fw.sequences[1]["poses"].shape == (5, 3, 4)
    fw5 = K.KittiOdometry(tmp_path, ["09"], seq_length=5)
    assert list(fw5.sequences[0]["first"]) == [0, 1]


def test_pose_statistics_reference_denominator():
    # two snippets (1, 2) and (3, 4) of a 4-frame sequence at seq_length 3: the reference's array has 4 rows, 2 of them zero
    E = np.array([[1.0, 2.0], [3.0, 4.0]])
    per = K.pose_statistics(E)
    ref = K.pose_statistics(E, 4)
    assert np.allclose(per["mean"], [2.0, 3.0]) and np.allclose(per["std"], [1.0, 1.0])
    assert np.allclose(ref["mean"], [1.0, 1.5])
    assert np.allclose(ref["std"], [np.sqrt((0 + 0 + 1 + 9) / 4.0 - 1.0), np.sqrt((0 + 0 + 4 + 16) / 4.0 - 2.25)])


# ------------------------------------------------------------------------------------------------------------------------- GPU
def _cuda(*arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


@pytest.mark.gpu
def test_entries_kitti_sizes_gpu():
    for name, H, W, n, seed in C.VELO_CASES[1:]:
        pts, P = C.velo_points(H, W, 20 * n, seed), C.P_velo2im(W, H)
        got = K.velo_depth(*_cuda(pts, P), H, W).cpu().numpy()
        assert _same_bits(got, R.velo_depth(pts, P, H, W)), name
    for name, h, w, H, W, seed in C.ZOOM_CASES[2:]:
        src = C.zoom_source(h, w, seed)
        got = K.spline_zoom(*_cuda(src), H, W, 1e-3, 80).cpu().numpy()
        assert _same_bits(got, R.spline_zoom(src, H, W, 1e-3, 80)), name
    gt = R.velo_depth(C.velo_points(375, 1242, 60000, 21), C.P_velo2im(1242, 375), 375, 1242)
    pred = R.spline_zoom(C.zoom_source(256, 832, 22), 375, 1242, 1e-3, 80)
    disp, norm = np.array([0.9, 1.1]), np.array([0.1, 0.12], np.float32)
    n = int(((gt > 1e-3) & (gt < 80) & R.crop_mask(375, 1242)).sum())
    assert n > 1000
    got = K.eigen_errors(*_cuda(gt, pred), 1e-3, 80, *_cuda(disp, norm)).cpu().numpy()
    _check_eigen(got, R.eigen_errors(gt, pred, 1e-3, 80, disp, norm), n)
    for name, L, mode, S, seed in C.POSE_CASES:
        pred, seq, first = C.pose_case(L, 200, seed)
        err, fin = K.pose_snippet_errors(*_cuda(pred, seq, first), mode, want_final=True)
        werr, wfin = R.pose_snippet_errors(pred, seq, first, mode)
        _rel(err.cpu().numpy(), werr, 1e-6)
        assert np.allclose(fin.cpu().numpy(), wfin, rtol=1e-6, atol=1e-6)


def _depth_sample(gt_pts, P, src, H, W, disp, norm):
    gt = K.velo_depth(gt_pts, P, H, W)
    z = K.spline_zoom(src, H, W, 1e-3, 80)
    return K.eigen_errors(gt, z, 1e-3, 80, disp, norm)


@pytest.mark.gpu
def test_run_to_run_and_graph_capture_gpu():
    H, W = 375, 1242
    ins = _cuda(C.velo_points(H, W, 60000, 31), C.P_velo2im(W, H), C.zoom_source(256, 832, 32), np.array([0.9, 0.0, 1.1]),
                np.array([0.1, 0.2, 0.12], np.float32))
    a = _depth_sample(ins[0], ins[1], ins[2], H, W, ins[3], ins[4]).clone()
    b = _depth_sample(ins[0], ins[1], ins[2], H, W, ins[3], ins[4]).clone()
    pa, sa, fa = _cuda(*C.pose_case(5, 300, 33))
    e1 = K.pose_snippet_errors(pa, sa, fa, "quat").clone()
    e2 = K.pose_snippet_errors(pa, sa, fa, "quat").clone()
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    assert torch.equal(e1.view(torch.int64), e2.view(torch.int64))
    static = [t.clone() for t in ins]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _depth_sample(static[0], static[1], static[2], H, W, static[3], static[4])
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = _depth_sample(static[0], static[1], static[2], H, W, static[3], static[4])
    new = _cuda(C.velo_points(H, W, 60000, 34), C.P_velo2im(W, H), C.zoom_source(256, 832, 35), np.array([0.7, 1.3, 0.0]),
                np.array([0.11, 0.09, 0.3], np.float32))
    for s, t in zip(static, new):
        s.copy_(t)
    graph.replay()
    eager = _depth_sample(*new[:3], H, W, new[3], new[4])
    torch.cuda.synchronize()
    assert torch.equal(captured.view(torch.int64), eager.view(torch.int64)), (captured, eager)


@pytest.mark.gpu
def test_evaluate_depth_end_to_end_gpu(tmp_path):
    from cc_amd import models
    from cc_amd.custom_transforms import DeviceFrames, _bytescale
    torch.manual_seed(0)
    files, (H, W) = make_raw_tree(tmp_path, H=40, W=120)
    dev = torch.device("cuda")
    disp_net = models.DispResNet6()
    disp_net.init_weights()
    disp_net.to(dev).eval()
    pose_net = models.PoseNetB6(nb_ref_imgs=2)
    pose_net.init_weights()
    pose_net.to(dev).eval()
    fw = K.KittiRawEigen(tmp_path, files, seq_length=3)
    hw = (64, 192)
    got, names = K.evaluate_depth(disp_net, fw, pose_net=pose_net, img_hw=hw)
    assert names == K.ERROR_NAMES and got.shape == (2, 7)
    # the same network outputs through the NumPy restatement
    frames = DeviceFrames(device=dev)
    want = []
    with torch.no_grad():
        for j in range(len(fw)):
            s = fw[j]
            x = frames.resize_crop(np.stack([_bytescale(f.astype(np.float32)) for f in [s["tgt"]] + s["ref"]]), hw, hw)
            depth = (1 / disp_net(x[:1])[0, 0]).cpu().numpy()
            norm = pose_net(x[:1], [x[1:2], x[2:3]])[0, :, :3].norm(2, 1).cpu().numpy()
            gt = R.velo_depth(s["velo"], s["P_velo2im"], H, W)
            want.append(R.eigen_errors(gt, R.spline_zoom(depth, H, W, 1e-3, 80), 1e-3, 80, s["displacements"], norm))
    n = min(int(((R.velo_depth(fw[j]["velo"], fw[j]["P_velo2im"], H, W) > 1e-3) & R.crop_mask(H, W)).sum()) for j in range(2))
    _check_eigen(got, np.mean(want, 0), max(n, 1))


@pytest.mark.gpu
def test_evaluate_pose_end_to_end_gpu(tmp_path):
    from cc_amd import models
    from cc_amd.custom_transforms import DeviceFrames, _bytescale
    torch.manual_seed(1)
    make_odometry_tree(tmp_path, H=40, W=120)
    dev = torch.device("cuda")
    pose_net = models.PoseNetB6(nb_ref_imgs=2)
    pose_net.init_weights()
    pose_net.to(dev).eval()
    fw = K.KittiOdometry(tmp_path, ["09", "1*"], seq_length=3)
    hw = (64, 192)
    res = K.evaluate_pose(pose_net, fw, "euler", img_hw=hw, batch_size=3)
    frames = DeviceFrames(device=dev)
    rows = []
    with torch.no_grad():
        for seq in fw.sequences:
            imgs = [K.imread(p) for p in seq["img_files"]]
            x = frames.resize_crop(np.stack([_bytescale(f.astype(np.float32)) for f in imgs]), hw, hw)
            preds = np.stack([pose_net(x[f + 1:f + 2], [x[f:f + 1], x[f + 2:f + 3]])[0].cpu().numpy() for f in seq["first"]])
            rows.append(R.pose_snippet_errors(preds, seq["poses"], seq["first"], "euler")[0])
    E = np.concatenate(rows)
    assert res["errors"].shape == E.shape == (len(fw), 2)
    # batched (3 snippets) and single-snippet network calls may differ in the last bits of the poses
    assert np.allclose(res["errors"], E, rtol=1e-4, atol=1e-6)
    assert np.allclose(res["per_snippet"]["mean"], E.mean(0), rtol=1e-4)
    padded = np.concatenate([E, np.zeros((fw.n_frames - len(fw), 2))])
    assert np.allclose(res["reference"]["mean"], padded.mean(0), rtol=1e-4)
    assert np.allclose(res["reference"]["std"], padded.std(0), rtol=1e-4)
