"""KITTI 2015 flow and motion-segmentation evaluation (cc_amd/csrc/kitti_flow_eval.hip through cc_amd/kitti_eval.py; reference
test_flow.py, test_mask.py, datasets/validation_flow.py).

CPU: the kernel sources on x86 (tests/hipemu) and the NumPy restatement tests/kitti_flow_np.py against the reference-written
fixture tests/golden/kitti_flow_eval.npz (tools/make_kitti_flow_golden.py); the PNG decoder against a test-side encoder, Pillow's
high bytes and a byte-wise restatement of the PNG specification; the reader on a tiny synthetic KITTI 2015 tree; evaluate_mask
end to end with seeded networks.  GPU: the three entries at KITTI size, run-to-run bit equality, a graph capture of the
composition and the counts, and both evaluation loops end to end.

Every comparison of masks, counts and decoded flow is exact: they are integer or correctly rounded fp32 arithmetic on both
sides.  The flow errors of evaluate_flow are compared with validate_flow_with_gt fed by hand with the same tensors at relative
1e-6 (the engine against itself; only the host's fp64 summation is free)."""
import os
import types

import numpy as np
import pytest
import torch

import kitti_flow_cases as C
import kitti_flow_np as R
from cc_amd import kitti_eval as K


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "kitti_flow_eval.npz"))


@pytest.fixture
def emu():
    from hipemu.emu import emulated_engine
    with emulated_engine() as e:
        yield e


def _t(a, dev="cpu"):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _gold_mask(gold, name, key, h, w):
    return np.unpackbits(gold["%s_%s" % (name, key)])[:h * w].reshape(1, 1, h, w).astype(np.float32)


def _decode(png_bytes, dev="cpu"):
    ftype, rows, W = K.png16_scanlines(png_bytes)
    return K.png16_flow_decode(_t(ftype, dev)[None], _t(rows, dev)[None], W)[0].cpu().numpy(), (ftype, rows, W)


def _want_flow(samples):
    return np.stack([(samples[..., 0].astype(np.float64) - 2 ** 15) / 64.0, (samples[..., 1].astype(np.float64) - 2 ** 15) / 64.0,
                     samples[..., 2].astype(np.float64)]).astype(np.float32)


# ----------------------------------------------------------------------------------------------------- fixture sanity (CPU)
def test_cases_plant_the_branches():
    for name, h, w, Hg, Wg, seed in C.MASK_CASES:
        mask, cam, fwd = C.compose_inputs(h, w, seed)
        comp = 1 - (1 - mask[:, 1]) * (1 - mask[:, 2])
        assert (comp > 0.5).any() and (comp < 0.5).any()                          # mask values on both sides of 0.5
        d2 = ((cam - fwd) ** 2).sum(1)
        assert (d2 == 0).sum() > 10                                               # flow_cam == flow_fwd
        top = np.sort(d2.reshape(-1))[-2:]
        assert top[1] > 4 * top[0]                                                # one clear maximum
        obj, sem = C.gt_maps(Hg, Wg, seed)
        assert obj.max() > 1 and (obj == 0).any()                                 # object ids above 1
        assert (sem == 26).any() and (sem != 26).any()                            # car and not car
        assert ((sem == 26) & (obj > 1)).any() and ((sem == 26) & (obj == 0)).any()


def test_restatement_matches_reference(gold):
    for name, h, w, Hg, Wg, seed in C.MASK_CASES:
        mask, cam, fwd = C.compose_inputs(h, w, seed)
        obj, sem = C.gt_maps(Hg, Wg, seed)
        bare, census, combined = R.compose_norm(mask, cam, fwd, C.THRESH)
        for key, m in (("bare", bare), ("census", census), ("combined", combined)):
            assert _same_bits(m, _gold_mask(gold, name, key, h, w)), (name, key)
        counts = np.stack([R.mask_counts(obj, sem, m[0, 0]) for m in (combined, census, bare)])
        assert np.array_equal(counts, gold[name + "_counts"]), name
        if name + "_total_flow" in gold:
            for key, f in zip(("flow_fwd_non_rigid", "flow_fwd_rigid", "total_flow"), R.flows(combined, cam, fwd)):
                assert _same_bits(f, gold["%s_%s" % (name, key)]), key


# ----------------------------------------------------------------------------------------------------------- PNG decode (CPU)
@pytest.mark.parametrize("case", C.PNG_CASES, ids=[c[0] for c in C.PNG_CASES])
def test_png_decode_emulated(emu, case, tmp_path):
    from PIL import Image
    name, H, W, seed = case
    samples = C.flow_samples(H, W, seed)
    data = C.encode_png(samples)
    got, (ftype, rows, w) = _decode(data)
    assert w == W and list(ftype) == [y % 5 for y in range(H)] and rows.shape[1] % 8 == 0
    assert _same_bits(got, _want_flow(samples))                                   # the encoder's input, exactly
    path = tmp_path / "flow.png"
    path.write_bytes(data)
    with Image.open(str(path)) as im:                                             # Pillow: the high byte of every sample
        high = np.asarray(im.convert("RGB"))
    assert np.array_equal(high, (samples >> 8).astype(np.uint8))
    assert _same_bits(got, R.flow_from_bytes(R.png_unfilter(ftype, rows, W), W))   # the byte-wise restatement
    assert _same_bits(K.read_flow_png(path, "cpu").numpy(), got)
    # one filter type for every row, and a batch of two files
    for ft in range(5):
        one, _ = _decode(C.encode_png(samples, np.full(H, ft), idat_split=1))
        assert _same_bits(one, got), ft
    other = C.flow_samples(H, W, seed + 100)
    pair = [K.png16_scanlines(C.encode_png(s, (np.arange(H) + k) % 5)) for k, s in enumerate((samples, other))]
    both = K.png16_flow_decode(_t(np.stack([p[0] for p in pair])), _t(np.stack([p[1] for p in pair])), W).numpy()
    assert _same_bits(both[0], got) and _same_bits(both[1], _want_flow(other))


def test_png_rejects_other_formats(tmp_path):
    from PIL import Image
    samples = C.flow_samples(4, 5, 1)
    for kw in (dict(bit_depth=8), dict(colour_type=6), dict(colour_type=0), dict(interlace=1)):
        with pytest.raises(ValueError):
            K.png16_scanlines(C.encode_png(samples, **kw))
    Image.fromarray((samples >> 8).astype(np.uint8)).save(str(tmp_path / "rgb8.png"))
    Image.fromarray(samples[..., 0]).save(str(tmp_path / "gray16.png"))
    for name in ("rgb8.png", "gray16.png"):
        with pytest.raises(ValueError):
            K.read_flow_png(tmp_path / name, "cpu")
    with pytest.raises(ValueError):
        K.png16_scanlines(b"not a png at all")
    K.png16_scanlines(C.encode_png(samples))                                       # the accepted format parses


# -------------------------------------------------------------------------------------------------- kernels, emulated (CPU)
def _compose_and_count(dev, name, h, w, Hg, Wg, seed, counts=None):
    mask, cam, fwd = C.compose_inputs(h, w, seed)
    obj, sem = C.gt_maps(Hg, Wg, seed)
    r = K.rigidity_composition_norm(_t(mask, dev), _t(cam, dev), _t(fwd, dev), C.THRESH)
    counts = K.mask_iou_counts(_t(obj, dev), _t(sem, dev),
                               (r.rigidity_mask_combined[0, 0], r.rigidity_mask_census[0, 0], r.rigidity_mask[0, 0]), counts)
    return r, counts


def _check_against_gold(dev, gold, case):
    name, h, w, Hg, Wg, seed = case
    r, counts = _compose_and_count(dev, *case)
    for key, m in (("bare", r.rigidity_mask), ("census", r.rigidity_mask_census), ("combined", r.rigidity_mask_combined)):
        assert _same_bits(m.cpu().numpy(), _gold_mask(gold, name, key, h, w)), (name, key)
    assert counts.dtype == torch.int64 and np.array_equal(counts.cpu().numpy(), gold[name + "_counts"]), name
    mask, cam, fwd = C.compose_inputs(h, w, seed)
    want = R.flows(_gold_mask(gold, name, "combined", h, w), cam, fwd)
    for f, wnt in zip((r.flow_fwd_non_rigid, r.flow_fwd_rigid, r.total_flow), want):
        assert _same_bits(f.cpu().numpy(), wnt)
    return counts


@pytest.mark.parametrize("case", C.MASK_CASES, ids=[c[0] for c in C.MASK_CASES])
def test_compose_and_counts_emulated(emu, gold, case):
    _check_against_gold("cpu", gold, case)


def test_counts_accumulate_emulated(emu, gold):
    case = C.MASK_CASES[0]
    _, counts = _compose_and_count("cpu", *case)
    _, counts = _compose_and_count("cpu", *case, counts=counts)                     # the second call adds into the buffer
    assert np.array_equal(counts.numpy(), 2 * gold["small_counts"])
    # a skipped mask leaves its row alone; only some outputs wanted
    name, h, w, Hg, Wg, seed = case
    obj, sem = C.gt_maps(Hg, Wg, seed)
    r = K.rigidity_composition_norm(*[_t(a) for a in C.compose_inputs(h, w, seed)], C.THRESH, want=("rigidity_mask_census",))
    assert r.rigidity_mask is None and r.total_flow is None
    part = K.mask_iou_counts(_t(obj), _t(sem), (None, r.rigidity_mask_census[0, 0]))
    assert np.array_equal(part.numpy()[1], gold["small_counts"][1]) and not part.numpy()[[0, 2]].any()


def test_per_sample_maximum_emulated(emu):
    """B = 2: each sample is normalised by its own maximum (the reference's .max() spans the batch, and its batch is 1)"""
    mask, cam, fwd = C.compose_inputs(24, 40, 53, B=2)
    r = K.rigidity_composition_norm(_t(mask), _t(cam), _t(fwd), C.THRESH)
    for b in range(2):
        one = R.compose_norm(mask[b:b + 1], cam[b:b + 1], fwd[b:b + 1], C.THRESH)
        assert _same_bits(r.rigidity_mask_census[b:b + 1].numpy(), one[1])
        assert _same_bits(r.rigidity_mask_combined[b:b + 1].numpy(), one[2])
    assert not _same_bits(r.rigidity_mask_census[0].numpy(), r.rigidity_mask_census[1].numpy())


def test_degenerate_census_emulated(emu):
    mask, cam, fwd = C.compose_inputs(24, 40, 54, B=2)
    fwd[0] = cam[0]                                                               # max == 0: 0 / 0
    fwd[1, 0, 3, 5] = np.nan                                                      # a NaN wins the maximum
    r = K.rigidity_composition_norm(_t(mask), _t(cam), _t(fwd), C.THRESH)
    assert not r.rigidity_mask_census.numpy().any()
    assert _same_bits(r.rigidity_mask_combined.numpy(), r.rigidity_mask.numpy())
    bare, census, combined = R.compose_norm(mask, cam, fwd, C.THRESH)
    assert not census.any() and _same_bits(r.rigidity_mask.numpy(), bare)
    # the same through torch, statement for statement
    d = (torch.from_numpy(cam) - torch.from_numpy(fwd)).pow(2).sum(dim=1).unsqueeze(1).sqrt()
    for b in range(2):
        assert not (1 - d[b] / d[b].max() > C.THRESH).any()
    fwd[1, 0, 3, 5] = np.inf                                                      # inf / inf is NaN there, finite / inf is 0 elsewhere
    r = K.rigidity_composition_norm(_t(mask), _t(cam), _t(fwd), C.THRESH)
    assert _same_bits(r.rigidity_mask_census.numpy(), R.compose_norm(mask, cam, fwd, C.THRESH)[1])
    assert r.rigidity_mask_census[1].sum() == 24 * 40 - 1


def test_zoom_lookup_beyond_the_last_sample_emulated(emu):
    """256 -> 376 rows: 375 * (255 / 375) exceeds 255 in double, so SciPy's zoom fills the last row with cval 0 (class 1)"""
    idx = R.nearest_index(376, 256)
    assert idx[-1] == -1 and (idx[:-1] >= 0).all() and (R.nearest_index(375, 256) >= 0).all()
    r = np.random.RandomState(5)
    pred = (r.rand(256, 8) > 0.5).astype(np.float32)
    obj, sem = (r.rand(376, 12) > 0.5).astype(np.uint8), np.full((376, 12), 26, np.uint8)
    got = K.mask_iou_counts(_t(obj), _t(sem), (_t(pred),)).numpy()
    assert np.array_equal(got[0], R.mask_counts(obj, sem, pred))


# ------------------------------------------------------------------------------------------------------------ reader (CPU)
def _save(path, arr):
    from PIL import Image
    path.parent.mkdir(parents=True, exist_ok=True)
    Image.fromarray(arr).save(str(path))


P_RECT_02 = [721.5377, 0.0, 609.5593, 44.85728, 0.0, 721.5377, 172.854, 0.2163791, 0.0, 0.0, 1.0, 0.002745884]


def make_kitti2015_tree(root, H=40, W=120, n=2, seed=0, flat_frame=False):
    """a tiny KITTI 2015 tree: n samples with frames _08.._12, flow_occ, calib, semantic; obj_map for the even indices only"""
    r = np.random.RandomState(seed)
    truth = []
    for i in range(n):
        name = "%06d" % i
        frames = {}
        for k in (8, 9, 10, 11, 12):
            f = (r.rand(H, W, 3) * 255).astype(np.uint8)
            if not flat_frame:
                f = (f // 2 + 40).astype(np.uint8)                                # min..max well inside 0..255: byte-scaling shows
            frames[k] = f
            _save(root / "data_scene_flow_multiview" / "training" / "image_2" / ("%s_%02d.png" % (name, k)), f)
        flow = C.flow_samples(H, W, seed + 10 + i)
        p = root / "data_scene_flow" / "training" / "flow_occ" / (name + "_10.png")
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(C.encode_png(flow))
        obj, sem = C.gt_maps(H, W, seed + i)
        if i % 2 == 0:
            _save(root / "data_scene_flow" / "training" / "obj_map" / (name + "_10.png"), obj)
        _save(root / "semantic_labels" / "training" / "semantic" / (name + "_10.png"), sem)
        c = root / "data_scene_flow_calib" / "training" / "calib_cam_to_cam" / (name + ".txt")
        c.parent.mkdir(parents=True, exist_ok=True)
        c.write_text("calib_time: 09-Jan-2012 13:57:47\nP_rect_02: %s\nP_rect_03: %s\n"
                     % (" ".join("%.6e" % v for v in P_RECT_02), " ".join("%.6e" % (v + 1) for v in P_RECT_02)))
        truth.append(dict(frames=frames, flow=flow, obj=obj if i % 2 == 0 else np.ones((H, W), np.uint8), sem=sem))
    return truth


def test_kitti2015_reader(emu, tmp_path):
    from cc_amd.custom_transforms import DeviceFrames, Scale, ArrayToTensor, Normalize, Compose
    H, W = 40, 120
    truth = make_kitti2015_tree(tmp_path, H, W)
    fw = K.Kitti2015Flow(tmp_path, sequence_length=5, N=2, with_semantic=True)
    assert fw.seq_ids == [8, 9, 11, 12] and len(fw) == 2
    assert K.Kitti2015Flow(tmp_path, sequence_length=3).seq_ids == [9, 11] and len(K.Kitti2015Flow(tmp_path)) == 200
    p = fw.paths(1)
    assert p["tgt"] == tmp_path / "data_scene_flow_multiview/training/image_2/000001_10.png"
    assert [q.name for q in p["ref"]] == ["000001_08.png", "000001_09.png", "000001_11.png", "000001_12.png"]
    assert p["flow"] == tmp_path / "data_scene_flow/training/flow_occ/000001_10.png"
    assert p["calib"] == tmp_path / "data_scene_flow_calib/training/calib_cam_to_cam/000001.txt"
    assert p["obj_map"] == tmp_path / "data_scene_flow/training/obj_map/000001_10.png"
    assert p["semantic"] == tmp_path / "semantic_labels/training/semantic/000001_10.png"
    assert K.Kitti2015Flow(tmp_path, occ="flow_noc", phase="testing").paths(0)["flow"] == \
        tmp_path / "data_scene_flow/testing/flow_noc/000000_10.png"
    s0, s1 = fw[0], fw[1]
    assert np.array_equal(s0["tgt"], truth[0]["frames"][10])
    assert all(np.array_equal(a, truth[0]["frames"][k]) for a, k in zip(s0["ref"], (8, 9, 11, 12)))
    assert np.array_equal(s0["obj_map"], truth[0]["obj"]) and np.array_equal(s0["semantic"], truth[0]["sem"])
    assert not p["obj_map"].is_file() and s1["obj_map"].shape == (H, W) and (s1["obj_map"] == 1).all()      # the missing obj_map
    assert K.Kitti2015Flow(tmp_path, N=2)[0]["semantic"] is None
    K0 = np.array(P_RECT_02, np.float64).reshape(3, 4)[:, :3].astype(np.float32)
    assert s0["intrinsics"].dtype == np.float32 and np.array_equal(s0["intrinsics"], K0)
    with pytest.raises(IndexError):
        fw[2]
    # the loader tuple against the host transform classes (Scale always resizes: byte-scaling even at an equal size)
    frames_dev = DeviceFrames(device="cpu")
    for hw in ((H, W), (32, 96)):
        tgt, refs, Kt, Kinv, flow_gt, obj_gt, sem = K.kitti2015_item(s0, hw, frames_dev)
        floats = [f.astype(np.float32) for f in [s0["tgt"]] + s0["ref"]]
        imgs, Kw = Compose([Scale(hw[0], hw[1]), ArrayToTensor(), Normalize([0.5] * 3, [0.5] * 3)])(floats, np.copy(K0))
        assert tgt.shape == (1, 3) + hw and len(refs) == 4
        assert torch.equal(tgt[0], imgs[0]) and all(torch.equal(a[0], b) for a, b in zip(refs, imgs[1:]))
        assert Kt.dtype == torch.float32 and np.array_equal(Kt[0].numpy(), Kw)
        assert np.array_equal(Kinv[0].numpy(), np.linalg.inv(Kw)) and Kinv.dtype == torch.float32
        want_K = K0.copy()
        want_K[0] *= hw[1] / W
        want_K[1] *= hw[0] / H
        assert np.array_equal(Kw, want_K)
        assert flow_gt.shape == (1, 3, H, W) and _same_bits(flow_gt[0].numpy(), _want_flow(truth[0]["flow"]))
        assert obj_gt.shape == (1, H, W) and obj_gt.dtype == torch.float32 and np.array_equal(obj_gt[0].numpy(), truth[0]["obj"])
        assert sem.dtype == torch.uint8 and np.array_equal(sem.numpy() == 26, truth[0]["sem"] == 26)
    tgt_same = K.kitti2015_item(s0, (H, W), frames_dev)[0]
    plain = torch.from_numpy(s0["tgt"].transpose(2, 0, 1).astype(np.float32)) / 255
    assert not torch.equal(tgt_same[0], (plain - 0.5) / 0.5)                      # stretched to its own min..max
    assert tgt_same.min() == -1 and tgt_same.max() == 1


# --------------------------------------------------------------------------------------------------- evaluation loops
def _nets(dev):
    from cc_amd import models, synthetic as syn
    from oracle.make_golden import validate_net_tweak
    nets = [models.DispResNet6(), models.PoseNetB6(nb_ref_imgs=4), models.MaskNet6(nb_ref_imgs=4, output_exp=True),
            models.Back2Future(nlevels=6)]
    for n in nets:
        n.load_state_dict(syn.seeded_state_dict(n, 0))
    validate_net_tweak(nets[2])
    return [n.to(dev).eval() for n in nets]


def _mask_counts_by_restatement(nets, fw, hw, thresh, dev):
    """the same network outputs through the NumPy restatement of test_mask.py's arithmetic"""
    from cc_amd.custom_transforms import DeviceFrames
    frames_dev = DeviceFrames(device=dev)
    total = np.zeros((3, 6), np.int64)
    with torch.no_grad():
        for i in range(len(fw)):
            s = fw[i]
            item = K.kitti2015_item(s, hw, frames_dev, with_flow=False)
            exp, cam, fwd = [t.cpu().numpy() for t in K.mask_sample_outputs(*nets, item)]
            bare, census, combined = R.compose_norm(exp, cam, fwd, thresh)
            total += np.stack([R.mask_counts(s["obj_map"], s["semantic"], m[0, 0]) for m in (combined, census, bare)])
    return total


def _check_evaluate_mask(dev, tmp_path):
    H, W, hw = 90, 260, (64, 192)
    make_kitti2015_tree(tmp_path, H, W)
    nets = _nets(dev)
    fw = K.Kitti2015Flow(tmp_path, N=2, with_semantic=True)
    res = K.evaluate_mask(*nets, fw, img_hw=hw)                                   # THRESH = 0.94, the protocol's
    want = _mask_counts_by_restatement(nets, fw, hw, 0.94, dev)
    assert res["counts"].dtype == np.int64 and np.array_equal(res["counts"], want), (res["counts"], want)
    assert res["names"] == K.MASK_COUNT_NAMES and want.sum() > 0
    for k, name in enumerate(K.MASK_ROWS):
        c = want[k].astype(np.float64)
        bg, fg = c[0] / (c[0] + c[1] + c[2]), c[3] / (c[3] + c[4] + c[5])
        assert np.allclose(res[name], ((bg + fg) / 2, bg, fg), rtol=0, atol=0, equal_nan=True)
    return nets, fw, hw


def test_evaluate_mask_end_to_end_emulated(emu, tmp_path):
    _check_evaluate_mask("cpu", tmp_path)


def test_mask_ious():
    c = np.array([[6, 1, 1, 3, 2, 1], [1, 0, 0, 0, 0, 5], [2, 2, 0, 4, 0, 4]])
    out = K.mask_ious(c)
    assert out["full"] == ((0.75 + 0.5) / 2, 0.75, 0.5) and out["census"] == (0.5, 1.0, 0.0) and out["bare"] == (0.5, 0.5, 0.5)


def test_cli_parses_the_reference_flags():
    base = ["--kitti-dir", "K", "--pretrained-disp", "d", "--pretrained-pose", "p", "--pretrained-mask", "m", "--pretrained-flow", "f"]
    a = K.parser().parse_args(["flow"] + base)
    assert (a.THRESH, a.dispnet, a.posenet, a.masknet, a.flownet, a.nlevels, a.N) == \
        (0.01, "DispResNet6", "PoseNetB6", "MaskNet6", "Back2Future", 6, 200)
    a = K.parser().parse_args(["mask"] + base + ["--THRESH", "0.9", "--flownet", "FlowNetC6", "--nlevels", "5"])
    assert (a.command, a.THRESH, a.flownet, a.nlevels, a.kitti_dir, a.pretrained_mask) == ("mask", 0.9, "FlowNetC6", 5, "K", "m")
    assert K.parser().parse_args(["mask"] + base).THRESH == 0.94


# ------------------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_entries_kitti_size_gpu(gold):
    H, W = 375, 1242
    samples = C.flow_samples(H, W, 71)
    data = C.encode_png(samples)                                                  # all five filter types, cycling
    got, (ftype, rows, w) = _decode(data, "cuda")
    assert sorted(set(ftype.tolist())) == [0, 1, 2, 3, 4]
    assert _same_bits(got, _want_flow(samples))
    assert _same_bits(got, R.flow_from_bytes(R.png_unfilter(ftype, rows, W), W))
    for case in C.MASK_CASES:
        _check_against_gold("cuda", gold, case)
    name, h, w, Hg, Wg, seed = C.MASK_CASES[1]
    mask, cam, fwd = C.compose_inputs(h, w, 72, B=2)
    obj, sem = C.gt_maps(Hg, Wg, 72)
    r = K.rigidity_composition_norm(_t(mask, "cuda"), _t(cam, "cuda"), _t(fwd, "cuda"), C.THRESH)
    want = R.compose_norm(mask, cam, fwd, C.THRESH)
    for m, wnt in zip((r.rigidity_mask, r.rigidity_mask_census, r.rigidity_mask_combined), want):
        assert _same_bits(m.cpu().numpy(), wnt)
    counts = K.mask_iou_counts(_t(obj, "cuda"), _t(sem, "cuda"), [r.rigidity_mask_combined[1, 0], r.rigidity_mask_census[1, 0],
                                                                   r.rigidity_mask[1, 0]]).cpu().numpy()
    assert np.array_equal(counts, np.stack([R.mask_counts(obj, sem, want[k][1, 0]) for k in (2, 1, 0)]))


def _mask_sample(mask, cam, fwd, obj, sem, counts):
    r = K.rigidity_composition_norm(mask, cam, fwd, C.THRESH, want=("rigidity_mask", "rigidity_mask_census", "rigidity_mask_combined"))
    K.mask_iou_counts(obj, sem, (r.rigidity_mask_combined[0, 0], r.rigidity_mask_census[0, 0], r.rigidity_mask[0, 0]), counts)
    return r.rigidity_mask_combined


def _mask_inputs(seed):
    name, h, w, Hg, Wg, _ = C.MASK_CASES[1]
    return [_t(a, "cuda") for a in C.compose_inputs(h, w, seed) + C.gt_maps(Hg, Wg, seed)]


@pytest.mark.gpu
def test_run_to_run_and_graph_capture_gpu():
    ins = _mask_inputs(81)
    ca, cb = torch.zeros((3, 6), dtype=torch.int64, device="cuda"), torch.zeros((3, 6), dtype=torch.int64, device="cuda")
    a = _mask_sample(*ins, ca).clone()
    b = _mask_sample(*ins, cb).clone()
    data = C.encode_png(C.flow_samples(375, 1242, 82))
    d1, _ = _decode(data, "cuda")
    d2, _ = _decode(data, "cuda")
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(ca, cb) and ca.sum() > 0 and _same_bits(d1, d2)
    static = [t.clone() for t in ins]
    counts = torch.zeros((3, 6), dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _mask_sample(*static, counts)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = _mask_sample(*static, counts)
    new = _mask_inputs(83)
    for s, t in zip(static, new):
        s.copy_(t)
    counts.zero_()
    graph.replay()
    graph.replay()                                                                # the counts add up over replays
    eager_counts = torch.zeros((3, 6), dtype=torch.int64, device="cuda")
    eager = _mask_sample(*new, eager_counts)
    torch.cuda.synchronize()
    assert torch.equal(captured, eager) and not torch.equal(eager, a)
    assert torch.equal(counts, 2 * eager_counts), (counts, eager_counts)


@pytest.mark.gpu
def test_evaluate_flow_and_mask_end_to_end_gpu(tmp_path):
    from cc_amd import validate as V
    from cc_amd.custom_transforms import DeviceFrames
    nets, fw, hw = _check_evaluate_mask("cuda", tmp_path)
    got, names = K.evaluate_flow(*nets, K.Kitti2015Flow(tmp_path, N=2), THRESH=0.01, img_hw=hw)
    assert names == K.FLOW_ERROR_NAMES and got.shape == (8,) and got.dtype == np.float64
    # validate_flow_with_gt fed by hand with the same tensors
    frames_dev = DeviceFrames(device="cuda")
    items = [K.kitti2015_item(fw[i], hw, frames_dev)[:6] for i in range(2)]
    want, _ = V.validate_flow_with_gt(items, *nets, args=types.SimpleNamespace(THRESH=0.01, flownet="Back2Future",
                                                                              spatial_normalize=False))
    want = np.asarray(want, dtype=np.float64)
    assert np.all(np.isfinite(want)) and np.all(np.abs(got - want) <= 1e-6 * np.abs(want)), (got, want)
