"""Shared cases of the ragged-batch flow metrics (metrics.flow_metrics_samples), the validation folder, the resident validation
stores and the loops over them (cc_amd/datasets/validation.py, cc_amd/validate.py): the synthetic trees
(tools/make_validation_golden.py builds the same depth tree for the fixture) and the checks that run on the x86 emulation build
(dev = "cpu") and on the GPU (dev = "cuda") alike."""
import json
import os
import types

import numpy as np
import pytest
import torch

import kitti_flow_cases as KC
from cc_amd import custom_transforms as CT
from cc_amd import datasets as DS
from cc_amd import kitti_eval as K
from cc_amd import metrics as M
from cc_amd import validate as V

# ----------------------------------------------------------------------------- the ragged batch
GT_SIZES = ((37, 124), (40, 120), (38, 123), (9, 20))          # the last: 180 pixels, one workgroup
PRED_HW = (16, 40)
IDX = ((3, 1, 0, 1), (2, 0, 3, 2))                             # permutations with a repeated row; between them every size
BIG_SIZES = ((375, 1242), (370, 1224))                         # 1820 and 1770 workgroups' worth of pixels: the 512 cap, grid stride
BIG_PRED_HW = (256, 832)


def _same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


_cases = {}


def ragged_case(sizes, pred_hw, B, seed):
    """host tensors, made once per key and never modified: per table row its gt [1,3,Hg,Wg] (validity zeros planted) and object
    map [1,Hg,Wg] (ids 0..3, so 1 - obj lies on both sides of THRESH), both also in the two pools, with a gap of unused floats
    before every sample; predictions [B,2,Hp,Wp] scaled so that outliers and inliers both occur; a dense mask around THRESH."""
    key = (sizes, pred_hw, B, seed)
    if key in _cases:
        return _cases[key]
    r = np.random.RandomState(seed)
    Hp, Wp = pred_hw
    gts, objs, table, fpool, opool = [], [], [], [], []
    for n, (Hg, Wg) in enumerate(sizes):
        gt = np.concatenate([r.randn(1, 2, Hg, Wg) * 6.0, (r.rand(1, 1, Hg, Wg) < 0.7)], 1).astype(np.float32)
        obj = KC.gt_maps(Hg, Wg, seed + n)[0].astype(np.float32)[None]
        fpool.append(np.full(5 + n, np.nan, np.float32))
        opool.append(np.full(3 + 2 * n, np.nan, np.float32))
        table.append((sum(a.size for a in fpool), sum(a.size for a in opool), Hg, Wg))
        fpool.append(gt.reshape(-1))
        opool.append(obj.reshape(-1))
        gts.append(torch.from_numpy(gt))
        objs.append(torch.from_numpy(obj))
    c = types.SimpleNamespace(
        gts=gts, objs=objs, flow_pool=torch.from_numpy(np.concatenate(fpool)), obj_pool=torch.from_numpy(np.concatenate(opool)),
        table=torch.tensor(table, dtype=torch.int64), max_px=max(h * w for h, w in sizes),
        rigid=torch.from_numpy((r.randn(B, 2, Hp, Wp) * 3.0).astype(np.float32)),
        nonrigid=torch.from_numpy((r.randn(B, 2, Hp, Wp) * 3.0).astype(np.float32)),
        mask=torch.from_numpy(r.rand(B, 1, Hp, Wp).astype(np.float32)))
    _cases[key] = c
    return c


def _samples_call(c, idx, dev, acc=None):
    d = lambda t: t.to(dev)
    return M.flow_metrics_samples(d(c.flow_pool), d(c.obj_pool), d(c.table), torch.tensor(idx, dtype=torch.int32, device=dev),
                                  d(c.rigid), d(c.nonrigid), d(c.mask), c.max_px, THRESH=0.5, acc=acc)


def _one_sample(c, row, b, dev):
    """the existing entry at B = 1 on sample `row`'s ground truth and the b-th slices of the predictions"""
    d = lambda t: t.to(dev).contiguous()
    return M.flow_metrics(d(c.gts[row]), d(c.rigid[b:b + 1]), d(c.nonrigid[b:b + 1]), masks=(d(c.mask[b:b + 1]), ("1-", d(c.objs[row]))),
                          THRESH=0.5)


def check_planted(c):
    for gt, obj in zip(c.gts, c.objs):
        assert (gt[:, 2] == 0).any() and (gt[:, 2] == 1).any()                  # validity zeros
        assert (1 - obj > 0.5).any() and (1 - obj < 0.5).any() and obj.max() > 1  # the inverted object map on both sides of THRESH
    assert (c.mask > 0.5).any() and (c.mask < 0.5).any()
    small = [h * w for h, w in GT_SIZES]
    assert min(small) < 256 < sorted(small)[1]                                  # one workgroup, and several


def check_rows_exact(dev, sizes=GT_SIZES, pred_hw=PRED_HW, idx_lists=IDX, seed=5):
    """1.: every row of the ragged call equals the existing entry at B = 1 on that sample's slices, byte for byte"""
    B = len(idx_lists[0])
    c = ragged_case(sizes, pred_hw, B, seed)
    check_planted(c)
    seen = set()
    for idx in idx_lists:
        got = _samples_call(c, idx, dev)
        assert got.shape == (B, 8) and got.dtype == torch.float32 and got.device.type == torch.device(dev).type
        for b, row in enumerate(idx):
            want = _one_sample(c, row, b, dev)
            assert _same_bits(got[b], want), (idx, b, got[b].tolist(), want.tolist())
            assert bool(torch.isfinite(got[b]).all()) and 0 < float(got[b, 3]) < 1 and 0 < float(got[b, 7]) < 1   # outliers and inliers
            seen.add(row)
        assert _same_bits(got, _samples_call(c, idx, dev))                     # run to run
    assert seen == set(range(len(sizes)))
    # a row the table does not hold, and a sample larger than max_px, give NaN rows and leave the others alone
    idx = list(idx_lists[0])
    good = _samples_call(c, idx, dev)
    bad = _samples_call(c, [len(sizes)] + idx[1:], dev)
    assert bool(torch.isnan(bad[0]).all()) and _same_bits(bad[1:], good[1:])
    c2 = types.SimpleNamespace(**dict(vars(c), max_px=min(h * w for h, w in sizes) + 1))
    small = _samples_call(c2, idx, dev)
    for b, row in enumerate(idx):
        if sizes[row][0] * sizes[row][1] > c2.max_px:
            assert bool(torch.isnan(small[b]).all())
        else:
            assert _same_bits(small[b], good[b])


def check_rows_against_oracle(dev, tol, sizes=GT_SIZES, pred_hw=PRED_HW, idx_lists=IDX, seed=5):
    """2.: the same rows against the restated reference arithmetic (oracle.metrics.compute_all_epes per sample), under the bar
    tests/test_metrics.py sets for the flow metrics: max |a - b| <= tol * max(1, max |b|), tol = 1e-6 on the host and 2e-5 on
    the device"""
    from oracle import metrics as OM
    c = ragged_case(sizes, pred_hw, len(idx_lists[0]), seed)
    for idx in idx_lists:
        got = _samples_call(c, idx, dev).cpu().numpy().astype(np.float64)
        for b, row in enumerate(idx):
            for k, m in enumerate((c.mask[b:b + 1], 1 - c.objs[row][None])):
                want = np.asarray([float(v) for v in OM.compute_all_epes(c.gts[row], c.rigid[b:b + 1], c.nonrigid[b:b + 1], m)])
                a = got[b, 4 * k:4 * k + 4]
                assert np.max(np.abs(a - want)) <= tol * max(1.0, np.max(np.abs(want))), (idx, b, k, a, want)


def check_meter(dev):
    """3.: two calls with acc: the sums are the sequential fp64 sum of the returned fp32 rows in order, the count their number"""
    c = ragged_case(GT_SIZES, PRED_HW, len(IDX[0]), 5)
    acc = M.ErrorSums(dev)
    rows = [_samples_call(c, idx, dev, acc=acc).cpu().numpy() for idx in IDX]
    want = np.zeros(8, dtype=np.float64)
    for out in rows:
        for b in range(out.shape[0]):
            for j in range(8):
                want[j] = want[j] + np.float64(out[b, j])
    n = sum(len(r) for r in rows)
    assert acc.sums.dtype == torch.float64 and acc.count.dtype == torch.int64
    assert np.array_equal(acc.sums.cpu().numpy().view(np.int64), want.view(np.int64)) and int(acc.count.cpu()[0]) == n
    means, count, flag = acc.read(extra=torch.ones((), dtype=torch.bool, device=dev))
    assert count == n and flag is True and means == [float(w) / n for w in want]
    empty = M.ErrorSums(dev).read()
    assert empty[1] == 0 and all(np.isnan(empty[0]))
    for idx in IDX:                                                             # without acc: the same rows
        assert _same_bits(_samples_call(c, idx, dev), torch.from_numpy(rows[IDX.index(idx)]))


def check_argument_errors(dev):
    """4.: CC_ERR_ARG (-1) for null pointers, B <= 0 and a maximum below 1; a size query of 0 for the same"""
    from cc_amd._lib import engine, STREAM
    E = engine()
    c = ragged_case(GT_SIZES, PRED_HW, 4, 5)
    d = lambda t: t.to(dev)
    fp, op, tb = d(c.flow_pool), d(c.obj_pool), d(c.table)
    idx = torch.tensor(IDX[0], dtype=torch.int32, device=dev)
    rg, nr, mk = d(c.rigid), d(c.nonrigid), d(c.mask)
    out = torch.empty(4, 8, device=dev)
    ws = torch.empty(E.call("cc_flow_metrics_samples_ws", 4, c.max_px), dtype=torch.uint8, device=dev)
    assert ws.numel() == 4 * min(512, -(-c.max_px // 256)) * 14 * 8
    sums, count = torch.zeros(8, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)

    def call(**kw):
        a = dict(fp=fp, op=op, tb=tb, N=4, idx=idx, B=4, max_px=c.max_px, rg=rg, nr=nr, mk=mk, out=out, sums=None, count=None, ws=ws)
        a.update(kw)
        E.call("cc_flow_metrics_samples", a["fp"], fp.numel(), a["op"], op.numel(), a["tb"], a["N"], a["idx"], a["B"], a["max_px"], a["rg"],
               a["nr"], PRED_HW[0], PRED_HW[1], a["mk"], PRED_HW[0], PRED_HW[1], 0.5, 3.0, 0.05, a["out"], a["sums"], a["count"], a["ws"],
               STREAM)

    call()
    call(sums=sums, count=count)
    for bad in (dict(fp=None), dict(op=None), dict(tb=None), dict(idx=None), dict(rg=None), dict(nr=None), dict(mk=None), dict(out=None),
                dict(ws=None), dict(B=0), dict(B=-1), dict(max_px=0), dict(max_px=-5), dict(N=0), dict(sums=sums), dict(count=count)):
        with pytest.raises(RuntimeError, match="code -1"):
            call(**bad)
    assert E.call("cc_flow_metrics_samples_ws", 0, c.max_px) == 0 and E.call("cc_flow_metrics_samples_ws", 4, 0) == 0


# ----------------------------------------------------------------------------- the depth validation folder
VAL_SCENES = (("scene_z", (10, 2, 7)), ("scene_a", (5, 1)))    # val.txt order (not sorted); frame numbers in the order written
OFF_LIST = ("scene_m", (0,))                                   # on the disk, not in val.txt
VH, VW = 40, 56
MEAN, STD = (0.5, 0.45, 0.4), (0.5, 0.25, 0.2)


def val_frame(scene, i, H=VH, W=VW):
    r = np.random.RandomState(7000 + 100 * scene + i)
    coarse = r.rand((H + 7) // 8 + 1, (W + 7) // 8 + 1, 3)
    fine = np.kron(coarse, np.ones((8, 8, 1)))[:H, :W] * 0.8 + r.rand(H, W, 3) * 0.2
    return (30.0 + fine * 200.0).astype(np.uint8)


def val_depth(scene, i, H=VH, W=VW):
    """float64 on the disk (the data set casts to float32): depths 0..100 m, a third of them 0 (no measurement)"""
    r = np.random.RandomState(9000 + 100 * scene + i)
    d = r.rand(H, W) * 100.0
    d[r.rand(H, W) < 0.33] = 0.0
    return d


def build_val_tree(root, H=VH, W=VW, final_newline=False):
    """root/val.txt (no newline after the last scene unless asked for), root/<scene>/<%07d>.jpg + .npy, a stray text file and a
    .png in the first scene, and one scene the list does not name"""
    from PIL import Image
    root = str(root)
    os.makedirs(root, exist_ok=True)
    for s, (name, numbers) in enumerate(VAL_SCENES + (OFF_LIST,)):
        d = os.path.join(root, name)
        os.makedirs(d, exist_ok=True)
        for i in numbers:
            Image.fromarray(val_frame(s, i, H, W), mode="RGB").save(os.path.join(d, "%07d.jpg" % i), quality=75)
            np.save(os.path.join(d, "%07d.npy" % i), val_depth(s, i, H, W))
    with open(os.path.join(root, VAL_SCENES[0][0], "cam.txt"), "w") as f:
        f.write("1,0,0\n0,1,0\n0,0,1\n")
    Image.fromarray(val_frame(0, 99, H, W), mode="RGB").save(os.path.join(root, VAL_SCENES[0][0], "0000099.png"))
    with open(os.path.join(root, "val.txt"), "w") as f:
        f.write("\n".join(name for name, _ in VAL_SCENES) + ("\n" if final_newline else ""))
    return root


def rel_names(root, paths):
    return [os.path.relpath(str(p), str(root)).replace(os.sep, "/") for p in paths]


def check_validation_set(root, golden_dir):
    """5.: the order against the fixture the unmodified reference wrote; items are Pillow's decode and the float32 depth"""
    from frame_store_cases import pillow_float
    gold = json.load(open(os.path.join(golden_dir, "validation_folder.json")))
    assert not open(os.path.join(root, "val.txt")).read().endswith("\n")
    ds = DS.ValidationSet(root)
    assert ds.scenes == gold["scenes"] == [n for n, _ in VAL_SCENES]
    assert rel_names(root, ds.imgs) == gold["imgs"] and rel_names(root, ds.depth) == gold["depth"] and len(ds) == len(gold["imgs"]) == 5
    assert gold["imgs"][0] == "scene_z/0000002.jpg" and gold["imgs"][3] == "scene_a/0000001.jpg"
    img, depth = ds[1]
    assert img.dtype == np.float32 and np.array_equal(img, pillow_float(ds.imgs[1]))
    assert depth.dtype == np.float32 and np.array_equal(depth, val_depth(0, 7).astype(np.float32))
    seen = []
    t = DS.ValidationSet(root, transform=lambda imgs, K: (seen.append((len(imgs), K)) or [imgs[0] * 2], K))
    assert np.array_equal(t[0][0], img_of(root, 0) * 2) and seen == [(1, None)]
    os.remove(os.path.join(root, "scene_a", "0000005.npy"))
    with pytest.raises(FileNotFoundError, match="0000005.npy"):
        DS.ValidationSet(root)


def img_of(root, k):
    from frame_store_cases import pillow_float
    return pillow_float(DS.ValidationSet(root).imgs[k])


def host_depth_batches(root, batch_size):
    ds = DS.ValidationSet(root, CT.Compose([CT.ArrayToTensor(), CT.Normalize(MEAN, STD)]))
    return list(torch.utils.data.DataLoader(ds, batch_size=batch_size, shuffle=False))


class TinyDisp(torch.nn.Module):
    """a stand-in with DispNet's contract ([B,3,H,W] -> positive [B,1,H,W]) at any size, seeded"""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(3)
        self.conv = torch.nn.Conv2d(3, 1, 3, padding=1)
        with torch.no_grad():
            self.conv.weight.copy_(torch.randn(self.conv.weight.shape, generator=g) * 0.3)
            self.conv.bias.fill_(0.1)

    def forward(self, x):
        return torch.sigmoid(self.conv(x)) * 0.3 + 0.01


def check_depth_store(dev, tmp_path):
    """6."""
    root = build_val_tree(tmp_path / "val")
    store = DS.DepthValStore.build(root, device=dev, workers=3, chunk_frames=2)
    assert tuple(store.frames.shape) == (5, VH, VW, 3) and store.frames.dtype == torch.uint8 and tuple(store.depth.shape) == (5, VH, VW)
    assert store.depth.dtype == torch.float32 and store.frames.device.type == store.depth.device.type == torch.device(dev).type
    assert store.names == rel_names(root, DS.ValidationSet(root).imgs) and len(store) == 5
    assert store.nbytes == 5 * VH * VW * 3 + 4 * 5 * VH * VW
    host = host_depth_batches(root, 2)
    loader = DS.DeviceDepthValLoader(store, 2, MEAN, STD)
    got = list(loader)
    assert len(got) == len(loader) == len(host) == 3 and got[-1][0].shape[0] == 1                 # the short last batch
    for (tgt, depth), (htgt, hdepth) in zip(got, host):
        assert tgt.dtype == torch.float32 and tgt.is_contiguous() and tgt.device.type == torch.device(dev).type
        assert tgt.shape == htgt.shape and _same_bits(tgt, htgt)
        assert depth.shape == hdepth.shape and hdepth.dtype == torch.float32 and _same_bits(depth, hdepth)
    # the cache
    d = str(tmp_path / "cache")
    store.save(d, chunk_frames=2)
    back = DS.DepthValStore.load(d, device=dev, chunk_frames=3)
    assert torch.equal(back.frames, store.frames) and _same_bits(back.depth, store.depth) and back.names == store.names
    assert back.nbytes == store.nbytes and back.frames.device == store.frames.device
    hdr_path = os.path.join(d, "store.json")
    hdr = json.load(open(hdr_path))
    for key, bad in (("frames", [5, VH, VW + 1, 3]), ("depth", [4, VH, VW]), ("names", hdr["names"][:-1]), ("format", 0), ("kind", "flow_val"),
                     ("nbytes", hdr["nbytes"] - 1)):
        with open(hdr_path, "w") as f:
            json.dump(dict(hdr, **{key: bad}), f)
        with pytest.raises(ValueError):
            DS.DepthValStore.load(d, device=dev)
    # the two loops agree: only the summation is free (fp32 AverageMeter there, fp64 here)
    net = TinyDisp().to(dev)
    for B in (2, 5):
        want, names = V.validate_depth_with_gt(DS.DeviceDepthValLoader(store, B), net)
        got, gnames = V.validate_depth_from_store(store, net, B)
        want, got = np.asarray(want, np.float64), np.asarray(got, np.float64)
        assert names == gnames == V.DEPTH_ERROR_NAMES and np.all(np.isfinite(want)) and np.all(want[:3] > 0)
        assert np.all(np.abs(got - want) <= 1e-6 * np.abs(want)), (B, got, want)
    # limits
    DS.DepthValStore.build(root, device=dev, max_bytes=store.nbytes)
    with pytest.raises(ValueError, match="max_bytes"):
        DS.DepthValStore.build(root, device=dev, max_bytes=store.nbytes - 1)
    from PIL import Image
    Image.fromarray(val_frame(1, 5, VH, VW - 8), mode="RGB").save(os.path.join(root, "scene_a", "0000005.jpg"), quality=75)
    with pytest.raises(ValueError, match="40 x 48"):
        DS.DepthValStore.build(root, device=dev, chunk_frames=2)
    Image.fromarray(val_frame(1, 5), mode="RGB").save(os.path.join(root, "scene_a", "0000005.jpg"), quality=75)
    np.save(os.path.join(root, "scene_a", "0000005.npy"), val_depth(1, 5, VH - 1, VW))
    with pytest.raises(ValueError, match="depth map"):
        DS.DepthValStore.build(root, device=dev, chunk_frames=2)


# ----------------------------------------------------------------------------- the flow store
P_RECT_02 = [721.5377, 0.0, 609.5593, 44.85728, 0.0, 721.5377, 172.854, 0.2163791, 0.0, 0.0, 1.0, 0.002745884]
FLOW_SIZES = ((90, 260), (88, 256), (92, 250))                 # at the emulated end-to-end test's network size, 64 x 192
FLOW_HW = (64, 192)


def make_flow_tree(root, sizes, seed=0):
    """test_kitti_flow_eval.make_kitti2015_tree's layout with a size per sample (KITTI 2015 comes in four): frames _08.._12,
    flow_occ, calib; obj_map for the even indices only (a missing one reads as ones)"""
    from PIL import Image
    r = np.random.RandomState(seed)

    def save(path, arr):
        path.parent.mkdir(parents=True, exist_ok=True)
        Image.fromarray(arr).save(str(path))

    for i, (H, W) in enumerate(sizes):
        name = "%06d" % i
        for k in (8, 9, 10, 11, 12):
            save(root / "data_scene_flow_multiview" / "training" / "image_2" / ("%s_%02d.png" % (name, k)),
                 ((r.rand(H, W, 3) * 255).astype(np.uint8) // 2 + 40).astype(np.uint8))
        p = root / "data_scene_flow" / "training" / "flow_occ" / (name + "_10.png")
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(KC.encode_png(KC.flow_samples(H, W, seed + 10 + i)))
        if i % 2 == 0:
            save(root / "data_scene_flow" / "training" / "obj_map" / (name + "_10.png"), KC.gt_maps(H, W, seed + i)[0])
        c = root / "data_scene_flow_calib" / "training" / "calib_cam_to_cam" / (name + ".txt")
        c.parent.mkdir(parents=True, exist_ok=True)
        c.write_text("calib_time: 09-Jan-2012 13:57:47\nP_rect_02: %s\n" % " ".join("%.6e" % (v + i) for v in P_RECT_02))


def seeded_nets(dev):
    from cc_amd import models, synthetic as syn
    from oracle.make_golden import validate_net_tweak
    nets = [models.DispResNet6(), models.PoseNetB6(nb_ref_imgs=4), models.MaskNet6(nb_ref_imgs=4, output_exp=True),
            models.Back2Future(nlevels=6)]
    for n in nets:
        n.load_state_dict(syn.seeded_state_dict(n, 0))
    validate_net_tweak(nets[2])
    return [n.to(dev).eval() for n in nets]


def check_flow_store(dev, tmp_path, sizes=FLOW_SIZES, hw=FLOW_HW, batch=2, cache=True):
    """7."""
    make_flow_tree(tmp_path, sizes)
    n = len(sizes)
    fw = K.Kitti2015Flow(tmp_path, N=n)
    store = DS.FlowValStore.build(fw, hw, device=dev)
    assert len(store) == n and tuple(store.inputs.shape) == (5, n, 3) + tuple(hw) and store.max_px == max(h * w for h, w in sizes)
    assert np.array_equal(store.table_np[:, 2:], np.array(sizes)) and torch.equal(store.table.cpu(), torch.from_numpy(store.table_np))
    assert store.table.dtype == torch.int64 and store.rows.dtype == torch.int32 and store.rows.tolist() == list(range(n))
    px = [h * w for h, w in sizes]
    assert store.flow_pool.numel() == 3 * sum(px) and store.obj_pool.numel() == sum(px)
    assert store.nbytes == 4 * (store.inputs.numel() + 18 * n + 4 * sum(px)) + 36 * n
    # the loader's six-tuples are kitti2015_item's, bit for bit
    frames_dev = CT.DeviceFrames(device=dev)
    items = [K.kitti2015_item(fw[i], hw, frames_dev)[:6] for i in range(n)]
    got = list(DS.DeviceFlowValLoader(store))
    assert len(got) == n
    for i, (g, w) in enumerate(zip(got, items)):
        assert g[4].shape == (1, 3) + sizes[i] and g[5].shape == (1,) + sizes[i]
        for a, b in zip([g[0]] + list(g[1]) + list(g[2:]), [w[0]] + list(w[1]) + list(w[2:])):
            assert a.shape == b.shape and a.is_contiguous() and _same_bits(a, b), i
    assert (got[1][5] == 1).all() and got[0][5].max() > 1                       # the missing object map reads as ones
    with pytest.raises(ValueError):
        list(DS.DeviceFlowValLoader(store, 2))
    b2 = list(DS.DeviceFlowValLoader(store, batch).batches())
    assert [t[0].shape[0] for t in b2] == [batch] * (n // batch) + ([n % batch] if n % batch else [])
    assert all(t.is_contiguous() for bt in b2 for t in [bt[0]] + bt[1] + list(bt[2:])) and \
        b2[-1][4].tolist() == list(range((n - 1) // batch * batch, n))
    if cache:
        d = str(tmp_path / "flow_cache")
        store.save(d)
        back = DS.FlowValStore.load(d, device=dev)
        for name in ("inputs", "K", "Kinv", "flow_pool", "obj_pool", "table", "rows"):
            assert _same_bits(getattr(back, name).float() if name in ("table", "rows") else getattr(back, name),
                              getattr(store, name).float() if name in ("table", "rows") else getattr(store, name)), name
        assert back.nbytes == store.nbytes and back.max_px == store.max_px
        DS.FlowValStore.build(fw, hw, device=dev, max_bytes=store.nbytes)
        with pytest.raises(ValueError, match="max_bytes"):
            DS.FlowValStore.build(fw, hw, device=dev, max_bytes=store.nbytes - 1)
    # batch size 1 against today's path over the files
    nets = seeded_nets(dev)
    want, names = K.evaluate_flow(*nets, fw, THRESH=0.01, img_hw=hw)
    args = types.SimpleNamespace(THRESH=0.01, flownet="Back2Future", spatial_normalize=False)
    one, names1 = K.evaluate_flow(*nets, None, THRESH=0.01, img_hw=hw, store=store)     # validate_flow_from_store at batch size 1
    assert names1 == names == K.FLOW_ERROR_NAMES and one.dtype == np.float64 and one.shape == (8,) and np.all(np.isfinite(want))
    assert np.all(np.abs(one - want) <= 1e-6 * np.abs(want)), (one, want)
    with pytest.raises(ValueError):
        K.evaluate_flow(*nets, fw, THRESH=0.01, img_hw=hw, batch_size=2)
    # a ragged batch and a short one: every row is the existing entry at B = 1 on slices of the same batched predictions
    seen = []

    def on_batch(k, t):
        idx = t["idx"].tolist()
        assert t["rows"].shape == (len(idx), 8)
        for b, row in enumerate(idx):
            alone = M.flow_metrics(store.flow_gt(row), t["flow_cam"][b:b + 1].contiguous(), t["flow_fwd"][b:b + 1].contiguous(),
                                   masks=(t["rigidity_mask_combined"][b:b + 1].contiguous(), ("1-", store.obj_map(row))), THRESH=0.5)
            assert _same_bits(t["rows"][b], alone), (k, b)
        seen.append((idx, t["rows"].cpu().numpy().astype(np.float64)))

    many, _ = V.validate_flow_from_store(store, *nets, batch_size=batch, args=args, on_batch=on_batch)
    assert [s[0] for s in seen] == [list(range(lo, min(n, lo + batch))) for lo in range(0, n, batch)]
    total = np.zeros(8)
    for _, rows in seen:
        for row in rows:
            total = total + row
    assert np.array_equal(np.asarray(many), total / n) and np.all(np.isfinite(many))
    return one, np.asarray(many)
