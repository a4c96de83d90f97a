"""Shared cases of the data preparation (cc_amd/datasets/prepare.py, python -m cc_amd.prepare): a tiny KITTI raw tree and a tiny
Cityscapes tree from fixed seeds (tools/make_prepare_golden.py runs the unmodified reference script on the same trees and records
what it wrote: tests/golden/prepare_kitti.npz, prepare_cityscapes.npz, prepare_test_scenes.txt), and the checks that run on the x86
emulation build (dev = "cpu") and on the GPU (dev = "cuda") alike."""
import io
import json
import os

import numpy as np
import torch

KITTI_SRC, KITTI_HW = (30, 100), (16, 64)
CITY_SRC, CITY_HW = (64, 128), (16, 32)
POINTS = 4000
# (date, drive, frames, what it is there for)
DRIVES = (("2011_09_26", "2011_09_26_drive_0001_sync", 12, "plain; its camera 03 is the validation scene of both runs"),
          ("2011_09_26", "2011_09_26_drive_0005_sync", 6, "every frame in the static list: removed for fewer than three frames"),
          ("2011_09_26", "2011_09_26_drive_0117_sync", 8, "named in the reference's test list"),
          ("2011_09_28", "2011_09_28_drive_0001_sync", 9, "frames 2, 3 and 7 in the static list"),
          ("2011_09_30", "2011_09_30_drive_0020_sync", 5, "image_03 lacks frame 0: no scene of either camera"),
          ("2011_09_30", "2011_09_30_drive_0028_sync", 8, "plain"))
STATIC = {"2011_09_26_drive_0005_sync": range(6), "2011_09_28_drive_0001_sync": (2, 3, 7)}
NO_CAM3_FRAME0 = "2011_09_30_drive_0020_sync"
# city -> {sequence: frame numbers}: a gap (two connex runs), an odd run length (13), and a frame the camera file is named after
CITIES = {"aachen": {"000000": list(range(0, 13)) + list(range(20, 30))},
          "bonn": {"000001": list(range(5, 19)), "000002": list(range(0, 9))}}
RESIZE_CASES = ((3, 37, 123, 16, 48, 16), (2, 64, 128, 13, 26, 13), (2, 24, 80, 24, 80, 24), (2, 30, 100, 16, 64, 12), (1, 20, 40, 33, 70, 33))
RESIZE_CASES_BIG = ((2, 375, 1242, 256, 832, 256), (1, 1024, 2048, 171, 416, 128))


def texture(seed, H, W):
    """a seeded low-pass texture with a little noise, uint8 [H,W,3]"""
    r = np.random.RandomState(seed)
    coarse = r.rand((H + 7) // 8 + 1, (W + 7) // 8 + 1, 3)
    fine = np.kron(coarse, np.ones((8, 8, 1)))[:H, :W] * 0.92 + r.rand(H, W, 3) * 0.08
    return (20.0 + fine * 220.0).astype(np.uint8)


def _save_png(a, path):
    from PIL import Image
    Image.fromarray(a).save(path, format="PNG")


def velo_points(seed, H, W, n=POINTS):
    """raw velodyne rows (forward, left, up, reflectance) that cover the H x W source image of the synthetic calibration, a
    tenth of them behind the sensor"""
    r = np.random.RandomState(seed)
    d = r.uniform(3.0, 40.0, n)
    u, v = r.uniform(-0.08 * W, 1.08 * W, n), r.uniform(-0.12 * H, 1.12 * H, n)
    X, Y = (u - 0.496 * W) / (0.72 * W) * d, (v - 0.507 * H) / (2.38 * H) * d
    pts = np.stack([d, -X, -Y, r.rand(n)], 1)
    pts[r.rand(n) < 0.1, 0] *= -1.0
    return pts.astype(np.float32)


def _calib_texts(H, W, k):
    P = lambda tx: "%.12e %.12e %.12e %.12e %.12e %.12e %.12e %.12e %.12e %.12e %.12e %.12e" % (
        0.72 * W + k, 0.0, 0.496 * W, tx, 0.0, 2.38 * H - k, 0.507 * H, 0.0, 0.0, 0.0, 1.0, 2.7e-3)
    a, b = 0.01 + 0.002 * k, -0.007
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]) @ \
        np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    nums = lambda m: " ".join("%.12e" % v for v in np.asarray(m).reshape(-1))
    cam = "calib_time: 09-Jan-2012 13:57:47\ncorner_dist: 9.950000e-02\nR_rect_00: %s\nP_rect_02: %s\nP_rect_03: %s\n" % (
        nums(R), P(0.045 * W), P(-0.33 * W))
    V = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]]) @ R.T
    velo = "calib_time: 15-Mar-2012 11:37:16\nR: %s\nT: %s\ndelta_f: 0.000000e+00 0.000000e+00\n" % (nums(V), nums([-0.004, -0.07, -0.27]))
    return cam, velo


def build_kitti_tree(root, src_hw=KITTI_SRC):
    """root/<date>/{calib_cam_to_cam.txt, calib_velo_to_cam.txt, <drive>/{image_02,image_03}/data/*.png, oxts/data/*.txt,
    velodyne_points/data/*.bin}, root/static_frames.txt -> root"""
    root = str(root)
    H, W = src_hw
    for k, date in enumerate(sorted({d[0] for d in DRIVES})):
        os.makedirs(os.path.join(root, date), exist_ok=True)
        cam, velo = _calib_texts(H, W, k)
        with open(os.path.join(root, date, "calib_cam_to_cam.txt"), "w") as f:
            f.write(cam)
        with open(os.path.join(root, date, "calib_velo_to_cam.txt"), "w") as f:
            f.write(velo)
    for j, (date, drive, n, _) in enumerate(DRIVES):
        base = os.path.join(root, date, drive)
        for sub in ("image_02/data", "image_03/data", "oxts/data", "velodyne_points/data"):
            os.makedirs(os.path.join(base, sub), exist_ok=True)
        r = np.random.RandomState(50 + j)
        for i in range(n):
            fid = "%010d" % i
            for c in (2, 3):
                if drive == NO_CAM3_FRAME0 and c == 3 and i == 0:
                    continue
                _save_png(texture(10000 * j + 100 * c + i, H, W), os.path.join(base, "image_%02d" % c, "data", fid + ".png"))
            row = r.uniform(-1.0, 1.0, 30)
            row[8:11] = r.uniform(0.2, 2.6), r.uniform(-0.05, 0.05), r.uniform(-0.05, 0.05)      # forward, left, up speed
            with open(os.path.join(base, "oxts", "data", fid + ".txt"), "w") as f:
                f.write(" ".join("%.10e" % v for v in row) + "\n")
            velo_points(777 * j + i, H, W).tofile(os.path.join(base, "velodyne_points", "data", fid + ".bin"))
    with open(os.path.join(root, "static_frames.txt"), "w") as f:
        for drive, ids in STATIC.items():
            for i in ids:
                f.write("%s %s %010d\n" % (drive[:10], drive, i))
    return root


def build_cityscapes_tree(root, src_hw=CITY_SRC):
    """root/leftImg8bit_sequence/train/<city>/*.png, root/camera/train/<city>/*_camera.json, root/vehicle_sequence/train/<city>/*.json"""
    root = str(root)
    H, W = src_hw
    for c, (city, seqs) in enumerate(sorted(CITIES.items())):
        dirs = [os.path.join(root, sub, "train", city) for sub in ("leftImg8bit_sequence", "camera", "vehicle_sequence")]
        for d in dirs:
            os.makedirs(d, exist_ok=True)
        for s, (seq, frames) in enumerate(sorted(seqs.items())):
            r = np.random.RandomState(900 + 10 * c + s)
            with open(os.path.join(dirs[1], "%s_%s_%06d_camera.json" % (city, seq, frames[3])), "w") as f:
                json.dump({"extrinsic": {"baseline": 0.21, "pitch": 0.04, "roll": 0.0, "x": 1.7, "y": 0.1, "yaw": -0.01, "z": 1.22},
                           "intrinsic": {"fx": 1.1 * W + s, "fy": 1.09 * W - c, "u0": 0.51 * W, "v0": 0.5 * H + 0.25}}, f)
            for i in frames:
                _save_png(texture(100000 * (c + 1) + 1000 * s + i, H, W), os.path.join(dirs[0], "%s_%s_%06d_leftImg8bit.png" % (city, seq, i)))
                with open(os.path.join(dirs[2], "%s_%s_%06d_vehicle.json" % (city, seq, i)), "w") as f:
                    json.dump({"gpsHeading": 0.1, "gpsLatitude": 50.7, "gpsLongitude": 6.1, "outsideTemperature": 20.5,
                               "speed": float(r.uniform(0.2, 1.6)), "yawRate": 0.001}, f)
    return root


def listing(root):
    root = str(root)
    return sorted(os.path.relpath(os.path.join(d, n), root).replace(os.sep, "/") for d, _, names in os.walk(root) for n in names)


def read_text(path):
    with open(path) as f:
        return f.read()


RUNS = ("kitti_speed", "kitti_static", "cityscapes")


def load_golden(golden_dir, run):
    """-> {'listing': [..], 'train': text, 'val': text, 'cam': {scene: text}, 'img': {scene/frame: uint8}, 'npy': {scene/frame: fp32}}"""
    z = np.load(os.path.join(golden_dir, "prepare_cityscapes.npz" if run == "cityscapes" else "prepare_kitti.npz"))
    out = {"cam": {}, "img": {}, "npy": {}}
    for key in z.files:
        parts = key.split(":")
        if parts[0] != run:
            continue
        if parts[1] in ("listing", "train", "val"):
            out[parts[1]] = [str(v) for v in z[key]] if parts[1] == "listing" else str(z[key])
        else:
            out[parts[1]][parts[2]] = str(z[key]) if parts[1] == "cam" else z[key]
    return out


_sources = {}


def source_tree(tmp_root, kind, src_hw=None):
    """one KITTI / Cityscapes source tree per size and test session: built once, shared, never modified"""
    src_hw = src_hw or (KITTI_SRC if kind == "kitti" else CITY_SRC)
    key = (kind, src_hw)
    if key not in _sources:
        build = build_kitti_tree if kind == "kitti" else build_cityscapes_tree
        _sources[key] = build(os.path.join(str(tmp_root), "%s%dx%d" % (kind, src_hw[0], src_hw[1])), src_hw)
    return _sources[key]


def kitti_loader(src, golden_dir, run, hw=KITTI_HW, get_gt=True):
    from cc_amd.datasets import prepare as P
    return P.KittiRaw(src, os.path.join(golden_dir, "prepare_test_scenes.txt"),
                      static_frames=os.path.join(src, "static_frames.txt") if run == "kitti_static" else None,
                      height=hw[0], width=hw[1], get_gt=get_gt)


# ----------------------------------------------------------------------------- 1. the resize kernel against Pillow itself
def pillow_resize(a, h, w, h_keep):
    from PIL import Image
    return np.asarray(Image.fromarray(a).resize((w, h), Image.BILINEAR))[:h_keep]


def check_resize(dev, cases=RESIZE_CASES):
    from cc_amd.datasets import prepare as P
    for k, (N, H, W, h, w, h_keep) in enumerate(cases):
        src = np.random.RandomState(40 + k).randint(0, 256, (N, H, W, 3)).astype(np.uint8)
        got = P.resize_u8(torch.from_numpy(src).to(dev), h, w, h_keep)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (N, h_keep, w, 3) and got.device.type == torch.device(dev).type
        got = got.cpu().numpy()
        for n in range(N):
            want = pillow_resize(src[n], h, w, h_keep)
            bad = int((got[n] != want).sum())
            print("resize %s frame %d: %d of %d bytes differ" % ((N, H, W, h, w, h_keep), n, bad, want.size))
            assert bad == 0, ((N, H, W, h, w, h_keep), n, bad)


def check_resize_errors(dev):
    import pytest
    from cc_amd._lib import engine, STREAM
    from cc_amd.datasets import prepare as P
    E = engine()
    src = torch.zeros((1, 8, 12, 3), dtype=torch.uint8, device=dev)
    dst = torch.zeros((1, 4, 6, 3), dtype=torch.uint8, device=dev)
    ws = torch.zeros(int(E.call("cc_frames_resize_u8_ws", 1, 8, 6)), dtype=torch.uint8, device=dev)
    assert ws.numel() == 8 * 6 * 3
    (ht, KH), (vt, KV) = P._axis_table(12, 6, torch.device(dev)), P._axis_table(8, 4, torch.device(dev))
    good = [src, dst, ht, KH, vt, KV, ws, 1, 8, 12, 4, 6, 4, STREAM]
    E.call("cc_frames_resize_u8", *good)
    for pos, bad in ((12, 5), (0, None), (1, None), (2, None), (4, None), (6, None), (9, 0), (9, -3), (7, 0), (12, 0), (3, 0), (5, 0), (8, 0)):
        args = list(good)
        args[pos] = bad
        with pytest.raises(RuntimeError, match="code -1"):
            E.call("cc_frames_resize_u8", *args)
    with pytest.raises(ValueError):
        P.resize_u8(torch.zeros((1, 8, 12, 3), dtype=torch.float32, device=dev), 4, 6)


# ----------------------------------------------------------------------------- 2. / 3. end to end against the golden
def _jpeg_round_trip(a):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, format="JPEG")
    buf.seek(0)
    return np.asarray(Image.open(buf))


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_dump(dump, rec, gold, with_npy):
    """the folders under `dump` and the record `prepare` returned, against what the reference wrote"""
    from PIL import Image
    assert listing(dump) == gold["listing"]
    assert read_text(os.path.join(dump, "train.txt")) == gold["train"] and read_text(os.path.join(dump, "val.txt")) == gold["val"]
    assert gold["train"] and gold["val"]
    assert rec["train"] == gold["train"].split() and rec["val"] == gold["val"].split()
    scenes = sorted(gold["cam"])
    assert rec["scenes"] == scenes == sorted(rec["train"] + rec["val"])
    for s in scenes:
        assert read_text(os.path.join(dump, s, "cam.txt")) == gold["cam"][s], s
    # every array the reference handed to imsave, those of the scenes it removed afterwards included
    got = {"%s/%s" % (s, f): rec["kept"][s][i] for s in rec["kept"] for i, f in enumerate(rec["kept_ids"][s])}
    assert sorted(got) == sorted(gold["img"])
    for key, want in gold["img"].items():
        assert _same_bits(got[key], want), (key, int((got[key] != want).sum()))
    for s in scenes:
        assert rec["frames"][s] == rec["kept_ids"][s] == sorted(n[:-4] for n in os.listdir(os.path.join(dump, s)) if n.endswith(".jpg"))
        for i, f in enumerate(rec["frames"][s]):
            with Image.open(os.path.join(dump, s, f + ".jpg")) as im:
                assert im.format == "JPEG" and np.array_equal(np.asarray(im), _jpeg_round_trip(rec["kept"][s][i])), (s, f)
    npys = [n for n in gold["listing"] if n.endswith(".npy")]
    assert sorted(n[:-4] for n in npys) == sorted(gold["npy"]) and bool(npys) == with_npy
    for key, want in gold["npy"].items():
        d = np.load(os.path.join(dump, key + ".npy"))
        diff = int((d.view(np.uint32) != want.view(np.uint32)).sum()) if d.shape == want.shape and d.dtype == want.dtype else -1
        print("depth map %s: %d of %d values differ in their bits" % (key, diff, want.size))
        assert _same_bits(d, want), (key, diff)


def check_kitti(dev, tmp_root, tmp_path, golden_dir, run):
    from cc_amd.datasets import prepare as P
    src = source_tree(tmp_root, "kitti")
    dump = os.path.join(str(tmp_path), "dump_" + run)
    state = np.random.get_state()[1].copy()
    rec = P.prepare(kitti_loader(src, golden_dir, run), dump, device=dev, workers=3, chunk_frames=5, keep_frames=True)
    assert np.array_equal(np.random.get_state()[1], state)                       # the global generator is not touched
    gold = load_golden(golden_dir, run)
    check_dump(dump, rec, gold, with_npy=True)
    assert len(rec["scenes"]) >= 6 and not any(s.startswith(("2011_09_26_drive_0117", NO_CAM3_FRAME0)) for s in rec["kept"])
    if run == "kitti_static":
        assert "2011_09_26_drive_0005_sync_02" not in rec["scenes"] and rec["kept"].get("2011_09_26_drive_0005_sync_02") is None
        assert rec["frames"]["2011_09_28_drive_0001_sync_02"] == ["%010d" % i for i in (0, 1, 4, 5, 6, 8)]
    else:
        n_all = {d[1]: d[2] for d in DRIVES}
        assert any(0 < len(f) < n_all[s[:-3]] for s, f in rec["frames"].items())   # the speed rule skipped frames
    assert set(rec["seconds"]) == set(P.STAGES) and rec["stores"] == {}


def check_cityscapes(dev, tmp_root, tmp_path, golden_dir):
    from cc_amd.datasets import prepare as P
    src = source_tree(tmp_root, "cityscapes")
    dump = os.path.join(str(tmp_path), "dump_city")
    loader = P.Cityscapes(src, height=CITY_HW[0], width=CITY_HW[1])
    assert loader.keep_rows == 12
    rec = P.prepare(loader, dump, device=dev, workers=2, chunk_frames=4, keep_frames=True)
    gold = load_golden(golden_dir, "cityscapes")
    check_dump(dump, rec, gold, with_npy=False)
    assert all(a.shape[1:] == (12, 32, 3) for a in rec["kept"].values())
    assert {"aachen_000000_000000_0", "aachen_000000_000020_0", "bonn_000002_000000_1"} <= set(rec["kept"]) | set(rec["scenes"])


# ----------------------------------------------------------------------------- 4. the stores
def check_stores(dev, tmp_root, tmp_path, golden_dir, src_hw=KITTI_SRC, hw=KITTI_HW, batch=False):
    import pytest
    from cc_amd import datasets as DS
    from cc_amd.datasets import prepare as P
    src = source_tree(tmp_root, "kitti", src_hw)
    dump, cache = os.path.join(str(tmp_path), "dump"), os.path.join(str(tmp_path), "cache")
    loader = kitti_loader(src, golden_dir, "kitti_static", hw)
    with pytest.raises(ValueError, match="max_bytes"):
        P.prepare(loader, os.path.join(str(tmp_path), "refused"), store_cache=cache, device=dev, max_bytes=1000)
    assert not os.path.exists(cache)
    rec = P.prepare(loader, dump, store_cache=cache, sequence_length=5, device=dev, workers=3, chunk_frames=4, keep_frames=True)
    frame = {"%s/%s.jpg" % (s, f): rec["kept"][s][i] for s in rec["scenes"] for i, f in enumerate(rec["frames"][s])}
    for name, is_train in (("train", True), ("val_unsup", False)):
        got = DS.FrameStore.load(os.path.join(cache, name), device=dev)
        want = DS.FrameStore.build(dump, train=is_train, sequence_length=5, device=dev, workers=2)
        assert got.scenes == want.scenes == rec["train" if is_train else "val"]
        for field in ("intrinsics", "samples", "sample_scene"):
            assert torch.equal(getattr(got, field), getattr(want, field)), (name, field)
        assert len(got) == rec["stores"][name] > 0 and got.frames.shape == want.frames.shape
        # the frames are the resized ones, never JPEG-coded: the store built off the folders holds their decodes
        _, _, found = DS.crawl(dump, is_train, 5)
        fr = got.frames.cpu().numpy()
        for k, (_, paths) in enumerate(found):
            for j, p in enumerate(paths):
                rel = os.path.relpath(p, dump).replace(os.sep, "/")
                assert np.array_equal(fr[got.samples_np[k, j]], frame[rel]), (name, rel)
        assert not torch.equal(got.frames, want.frames)
        mm = got.minmax.cpu().numpy()
        assert np.array_equal(mm[:, 0], fr.reshape(len(fr), -1).min(1).astype(np.float32)) and \
            np.array_equal(mm[:, 1], fr.reshape(len(fr), -1).max(1).astype(np.float32))
    got = DS.DepthValStore.load(os.path.join(cache, "val_depth"), device=dev)
    want = DS.DepthValStore.build(dump, device=dev, workers=2)
    assert got.names == want.names and len(got) == rec["stores"]["val_depth"] > 0
    assert torch.equal(got.depth, want.depth) and tuple(got.depth.shape[1:]) == tuple(hw)
    assert all(np.array_equal(got.frames[i].cpu().numpy(), frame[n]) for i, n in enumerate(got.names))
    if batch:
        import random
        from cc_amd import custom_transforms as CT
        store = DS.FrameStore.load(os.path.join(cache, "train"), device=dev)
        random.seed(3)
        np.random.seed(3)
        out, Ks = CT.DeviceTrainTransform(device=dev).from_store(store, [0, len(store) - 1])
        assert tuple(out.shape) == (2, 5, 3) + tuple(hw) and bool(torch.isfinite(out).all()) and len(Ks) == 2


# ----------------------------------------------------------------------------- 5. the command line
def check_parser():
    from cc_amd import prepare as M
    p = M.build_parser()
    opts = {a.option_strings[0] if a.option_strings else a.dest: a for a in p._actions}
    want = {"--dataset-format": (None, str), "--static-frames": (None, None), "--with-gt": (False, None), "--dump-root": (None, str),
            "--height": (128, int), "--width": (416, int), "--num-threads": (4, int)}
    for flag, (default, typ) in want.items():
        assert opts[flag].default == default and opts[flag].type == typ, flag
    assert opts["--dataset-format"].choices == ["kitti", "cityscapes"] and opts["--dataset-format"].required and opts["--dump-root"].required
    assert opts["dataset_dir"].metavar == "DIR"
    a = p.parse_args(["D", "--dataset-format", "kitti", "--dump-root", "O"])
    assert (a.test_scenes, a.store_cache, a.sequence_length, a.device, a.chunk_frames) == (None, None, 5, "cuda", 64)


def check_cli_refuses_kitti_without_test_scenes(capsys):
    import pytest
    from cc_amd import prepare as M
    with pytest.raises(SystemExit):
        M.main(["D", "--dataset-format", "kitti", "--dump-root", "O"])
    assert "--test-scenes" in capsys.readouterr().err


def check_cli_run(dev, tmp_root, tmp_path, golden_dir, capsys):
    """the driver end to end on the KITTI tree: its JSON line, and the same folders as the library call"""
    from cc_amd import prepare as M
    src = source_tree(tmp_root, "kitti")
    dump = os.path.join(str(tmp_path), "cli")
    M.main([src, "--dataset-format", "kitti", "--dump-root", dump, "--height", "16", "--width", "64", "--with-gt", "--num-threads", "2",
            "--test-scenes", os.path.join(golden_dir, "prepare_test_scenes.txt"), "--device", dev, "--chunk-frames", "7"])
    out = capsys.readouterr().out.strip().splitlines()
    line = json.loads(out[-1])
    gold = load_golden(golden_dir, "kitti_speed")
    assert len(out) == 1 and line["scenes"] == len(gold["cam"]) and line["train"] + line["val"] == line["scenes"]
    assert line["frames"] == sum(1 for n in gold["listing"] if n.endswith(".jpg")) and set(line["seconds"]) >= {"decode", "resize", "encode"}
    assert listing(dump) == gold["listing"]
    dump2 = os.path.join(str(tmp_path), "cli_none")
    M.main([src, "--dataset-format", "kitti", "--dump-root", dump2, "--height", "16", "--width", "64", "--test-scenes", "none", "--device", dev])
    io_ = capsys.readouterr()
    assert sum("--test-scenes none" in line for line in io_.err.splitlines()) == 1
    assert os.path.isdir(os.path.join(dump2, "2011_09_26_drive_0117_sync_02"))


def check_grey_png(dev, tmp_path):
    import pytest
    from PIL import Image
    from cc_amd.datasets import prepare as P
    src = build_cityscapes_tree(os.path.join(str(tmp_path), "grey"))
    for i in CITIES["bonn"]["000002"]:                                            # whichever of them the speed rule keeps
        bad = os.path.join(src, "leftImg8bit_sequence", "train", "bonn", "bonn_000002_%06d_leftImg8bit.png" % i)
        Image.fromarray(np.full(CITY_SRC, 90, dtype=np.uint8)).save(bad, format="PNG")
    with pytest.raises(ValueError, match=r"bonn_000002_\d{6}_leftImg8bit\.png"):
        P.prepare(P.Cityscapes(src, height=CITY_HW[0], width=CITY_HW[1]), os.path.join(str(tmp_path), "dump_grey"), device=dev, workers=2)
