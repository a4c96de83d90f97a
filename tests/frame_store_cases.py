"""Shared cases of the sequence-folder data set, the resident frame store and the device loader (cc_amd/datasets):
the synthetic tree (tools/make_sequence_golden.py builds the same one for the fixture), the host pipeline every device result is
compared with, and the checks that run on the x86 emulation build (dev = "cpu") and on the GPU (dev = "cuda") alike."""
import json
import os
import random

import numpy as np
import torch

from cc_amd import custom_transforms as CT
from cc_amd import datasets as DS

SCENES = (("scene_a", 7), ("scene_b", 6), ("scene_c", 2))      # the third is skipped at sequence lengths 3 and 5
GREY = ("scene_a", 3)                                          # one constant frame: cmax == cmin
SEEDS, LENGTHS = (0, 3), (3, 5)
MEAN, STD = (0.5, 0.45, 0.4), (0.5, 0.25, 0.2)


def frame_pixels(scene, i, H, W):
    """a seeded low-pass texture with min > 0 and max < 255 (the byte-scale stretches it), or the constant frame"""
    if (SCENES[scene][0], i) == GREY:
        return np.full((H, W, 3), 128, dtype=np.uint8)
    r = np.random.RandomState(1000 * scene + i)
    coarse = r.rand((H + 7) // 8 + 1, (W + 7) // 8 + 1, 3)
    fine = np.kron(coarse, np.ones((8, 8, 1)))[:H, :W] * 0.8 + r.rand(H, W, 3) * 0.2
    return (50.0 + fine * 140.0).astype(np.uint8)


def scene_intrinsics(scene, H, W):
    return np.array([[(0.58 + 0.01 * scene) * W, 0, 0.49 * W], [0, (1.92 - 0.02 * scene) * H, 0.5 * H + scene], [0, 0, 1]], dtype=np.float32)


def build_tree(root, H=40, W=56):
    """root/train.txt (all scenes), root/val.txt (the last two), root/<scene>/{cam.txt, 0000000.jpg ...}, frames saved by Pillow"""
    from PIL import Image
    root = str(root)
    os.makedirs(root, exist_ok=True)
    for s, (name, n) in enumerate(SCENES):
        d = os.path.join(root, name)
        os.makedirs(d, exist_ok=True)
        K = scene_intrinsics(s, H, W)
        with open(os.path.join(d, "cam.txt"), "w") as f:
            f.write("\n".join(",".join(repr(float(v)) for v in row) for row in K) + "\n")
        for i in range(n):
            Image.fromarray(frame_pixels(s, i, H, W), mode="RGB").save(os.path.join(d, "%07d.jpg" % i), quality=75)
    with open(os.path.join(root, "train.txt"), "w") as f:
        f.write("".join(name + "\n" for name, _ in SCENES))
    with open(os.path.join(root, "val.txt"), "w") as f:
        f.write("".join(name + "\n" for name, _ in SCENES[1:]))
    return root


def pillow_float(path):
    from PIL import Image
    return np.asarray(Image.open(path)).astype(np.float32)


def rel_names(root, paths):
    return [os.path.relpath(p, str(root)).replace(os.sep, "/") for p in paths]


# ----------------------------------------------------------------------------- 1. crawler and order
def check_sequence_folder(root, golden_dir):
    gold = json.load(open(os.path.join(golden_dir, "sequence_folder.json")))
    assert gold["seeds"] == list(SEEDS) and gold["sequence_lengths"] == list(LENGTHS)
    for seed in SEEDS:
        for L in LENGTHS:
            ds = DS.SequenceFolder(root, seed=seed, train=True, sequence_length=L)
            want = gold["order"]["seed%d.len%d" % (seed, L)]
            got = [rel_names(root, [s["tgt"]] + s["ref_imgs"]) for s in ds.samples]
            assert got == want, (seed, L)
            assert len(ds) == len(want) == sum(n - (L - 1) for _, n in SCENES if n >= L)
            for s in ds.samples:
                scene = s["tgt"].split(os.sep)[-2]
                assert s["intrinsics"].dtype == np.float32
                assert np.array_equal(s["intrinsics"], np.array(gold["intrinsics"][scene], dtype=np.float32)), scene
    ds = DS.SequenceFolder(root, seed=3, train=True, sequence_length=5)
    for k in (0, len(ds) - 1):
        tgt, refs, K, Kinv = ds[k]
        s = ds.samples[k]
        assert tgt.dtype == np.float32 and tgt.shape == (40, 56, 3) and len(refs) == 4
        for a, p in zip([tgt] + refs, [s["tgt"]] + s["ref_imgs"]):
            assert np.array_equal(a, pillow_float(p)), p
        assert np.array_equal(K, s["intrinsics"]) and K is not s["intrinsics"] and np.array_equal(Kinv, np.linalg.inv(K))
    # the transform sees [tgt] + refs and the intrinsics; the reference order is -d .. -1, +1 .. +d
    scenes, intr, found = DS.crawl(root, True, 5)
    assert scenes == [n for n, _ in SCENES] and intr.shape == (3, 3, 3) and intr.dtype == np.float32
    sc, paths = found[0]
    assert sc == 0 and rel_names(root, paths) == ["scene_a/%07d.jpg" % i for i in (2, 0, 1, 3, 4)]
    seen = []
    ds = DS.SequenceFolder(root, seed=0, sequence_length=3, transform=lambda imgs, K: (seen.append(len(imgs)) or imgs[::-1], K * 2))
    tgt, refs, K, Kinv = ds[0]
    assert seen == [3] and np.array_equal(tgt, pillow_float(ds.samples[0]["ref_imgs"][-1])) and np.array_equal(K, ds.samples[0]["intrinsics"] * 2)
    val = DS.SequenceFolder(root, seed=0, train=False, sequence_length=3)
    assert {s["tgt"].split(os.sep)[-2] for s in val.samples} == {"scene_b"} and len(val) == 4


def check_bad_files(tmp_path):
    from PIL import Image
    import pytest
    root = build_tree(tmp_path / "bad")
    grey = os.path.join(root, "scene_b", "0000002.jpg")
    Image.fromarray(np.full((40, 56), 90, dtype=np.uint8), mode="L").save(grey, quality=75)
    ds = DS.SequenceFolder(root, seed=0, sequence_length=3)
    k = [i for i, s in enumerate(ds.samples) if s["tgt"] == grey][0]
    with pytest.raises(ValueError, match="RGB JPEG"):
        ds[k]
    Image.fromarray(frame_pixels(1, 2, 40, 56), mode="RGB").save(grey, format="PNG")          # a PNG under a .jpg name
    with pytest.raises(ValueError, match="RGB JPEG"):
        ds[k]
    with open(grey, "wb") as f:
        f.write(b"not an image")
    with pytest.raises(ValueError):
        ds[k]


# ----------------------------------------------------------------------------- 2. store build
def check_store_build(dev, tmp_path):
    import pytest
    root = build_tree(tmp_path / "tree")
    for L in LENGTHS:
        store = DS.FrameStore.build(root, train=True, sequence_length=L, device=dev, workers=3, chunk_frames=3)
        scenes, intr, found = DS.crawl(root, True, L)
        paths = sorted({p for _, ps in found for p in ps})
        F = len(paths)
        assert F == 13 and tuple(store.frames.shape) == (F, 40, 56, 3) and store.frames.dtype == torch.uint8      # 5 chunks of <= 3
        assert store.frames.device.type == torch.device(dev).type and store.minmax.device.type == torch.device(dev).type
        fr, mm = store.frames.cpu().numpy(), store.minmax.cpu().numpy()
        assert store.samples.dtype == torch.int32 and tuple(store.samples.shape) == (len(found), L) and len(store) == len(found)
        for k, (sc, ps) in enumerate(found):
            assert int(store.sample_scene[k]) == sc
            for j, p in enumerate(ps):
                assert np.array_equal(fr[int(store.samples[k, j])].astype(np.float32), pillow_float(p)), (k, j)
        assert sorted(set(store.samples_np.reshape(-1).tolist())) == list(range(F))                        # each distinct frame once
        assert mm.dtype == np.float32 and np.array_equal(mm[:, 0], fr.reshape(F, -1).min(1).astype(np.float32)) and \
            np.array_equal(mm[:, 1], fr.reshape(F, -1).max(1).astype(np.float32))
        assert int((mm[:, 0] == mm[:, 1]).sum()) == 1 and float(mm[:, 0].min()) > 0 and float(mm[:, 1].max()) < 255
        assert np.array_equal(store.intrinsics_np, intr) and store.scenes == scenes
        assert store.nbytes == F * 40 * 56 * 3 + 8 * F
    # the store's own cache: bit for bit, uploaded in chunks through the same staging buffers
    d = str(tmp_path / "cache")
    store.save(d, chunk_frames=4)
    back = DS.FrameStore.load(d, device=dev, chunk_frames=3)
    for name in ("frames", "minmax", "intrinsics", "samples", "sample_scene"):
        a, b = getattr(store, name), getattr(back, name)
        assert a.dtype == b.dtype and a.device == b.device and torch.equal(a, b), name
    assert back.scenes == store.scenes and back.nbytes == store.nbytes
    hdr_path = os.path.join(d, "store.json")
    hdr = json.load(open(hdr_path))
    for key, bad in (("frames", [F, 40, 57, 3]), ("samples", [hdr["samples"][0] + 1, 5]), ("scenes", hdr["scenes"][:-1]), ("format", 0),
                     ("nbytes", hdr["nbytes"] - 1)):
        with open(hdr_path, "w") as f:
            json.dump(dict(hdr, **{key: bad}), f)
        with pytest.raises(ValueError):
            DS.FrameStore.load(d, device=dev)
    need = store.nbytes
    DS.FrameStore.build(root, sequence_length=5, device=dev, workers=2, chunk_frames=3, max_bytes=need)
    with pytest.raises(ValueError, match="max_bytes"):
        DS.FrameStore.build(root, sequence_length=5, device=dev, workers=2, chunk_frames=3, max_bytes=need - 1)
    # frames of unequal size
    from PIL import Image
    Image.fromarray(frame_pixels(1, 4, 40, 48), mode="RGB").save(os.path.join(root, "scene_b", "0000004.jpg"), quality=75)
    with pytest.raises(ValueError, match="40 x 48"):
        DS.FrameStore.build(root, sequence_length=5, device=dev, workers=2, chunk_frames=3)


# ----------------------------------------------------------------------------- 3. store transform, bit for bit
_trees = {}


def tree_and_store(dev, tmp_root, H, W, L=5):
    """one tree and one store per (device, size, length) and test session: built once, shared, never modified"""
    key = (str(dev), H, W, L)
    if key not in _trees:
        root = build_tree(os.path.join(str(tmp_root), "tree_%dx%d" % (H, W)), H, W)
        _trees[key] = (root, DS.FrameStore.build(root, sequence_length=L, device=dev, workers=4, chunk_frames=3))
    return _trees[key]


def host_samples(store, root, ids, as_u8=False):
    """the decoded frames of samples `ids`, as the reference's loader hands them to the transforms (float32), or as uint8"""
    _, _, found = DS.crawl(root, True, store.samples.shape[1])
    out = []
    for k in ids:
        sc, ps = found[k]
        frames = [pillow_float(p) for p in ps]
        out.append(([f.astype(np.uint8) for f in frames] if as_u8 else frames, np.copy(store.intrinsics_np[sc])))
    return out


def host_pipeline(samples, rotate, tail, seed=11):
    """the host classes (pinned to the reference by tests/golden/transforms.npz) sample by sample under one seeding"""
    random.seed(seed)
    np.random.seed(seed)
    t = CT.Compose(([CT.RandomRotate()] if rotate else []) + [CT.RandomHorizontalFlip(), CT.RandomScaleCrop(), CT.ArrayToTensor()] + tail)
    return [t([f.copy() for f in frames], np.copy(K)) for frames, K in samples]


def store_ids(store):
    """out of order, one id twice, and samples that hold the constant frame"""
    S = len(store)
    ids = [S - 1, 1, 0, 1]
    grey = int(np.flatnonzero((store.minmax.cpu().numpy()[:, 0] == store.minmax.cpu().numpy()[:, 1]))[0])
    assert any(grey in store.samples_np[i] for i in ids)
    return ids


def check_store_transform(dev, tmp_root, sizes=((40, 56), (36, 52))):
    for (H, W) in sizes:
        root, store = tree_and_store(dev, tmp_root, H, W)
        ids = store_ids(store)
        for rotate in (False, True):
            for stretch in (True, False):
                host = host_pipeline(host_samples(store, root, ids, as_u8=not stretch), rotate, [CT.Normalize(mean=MEAN, std=STD)])
                tr = CT.DeviceTrainTransform(MEAN, STD, device=dev, rotate=rotate)
                random.seed(11)
                np.random.seed(11)
                out, Ks = tr.from_store(store, ids, stretch=stretch)
                assert out.shape == (len(ids), 5, 3, H, W) and out.dtype == torch.float32 and out.is_contiguous()
                for b, (imgs, K) in enumerate(host):
                    assert np.array_equal(np.asarray(K), np.asarray(Ks[b])), (H, W, rotate, stretch, b)
                    for i, im in enumerate(imgs):
                        assert torch.equal(out[b, i].cpu(), im), (H, W, rotate, stretch, b, i, float((out[b, i].cpu() - im).abs().max()))
                if stretch:
                    # the same draws as __call__ on the decoded frames of the same samples
                    random.seed(11)
                    np.random.seed(11)
                    dense, Kd = tr(host_samples(store, root, ids))
                    assert torch.equal(dense, out) and all(np.array_equal(a, b) for a, b in zip(Kd, Ks))
                    random.seed(11)
                    np.random.seed(11)
                    fm, Kf = tr.from_store(store, ids, frame_major=True)
                    assert fm.shape == (5, len(ids), 3, H, W) and torch.equal(fm.permute(1, 0, 2, 3, 4), out)
                    assert all(np.array_equal(a, b) for a, b in zip(Kf, Ks))
        # the repeated id gets the draws of its own position in the batch
        assert not torch.equal(out[1], out[3])


def check_store_to_tensor(dev, tmp_root):
    import pytest
    root, store = tree_and_store(dev, tmp_root, 36, 52)
    prep = CT.DeviceFrames(mean=MEAN, std=STD, device=dev)
    idx, flips, offs, hw = [12, 3, 0, 3], [1, 0, 1, 0], [(3, 5), (0, 0), (4, 20), (2, 1)], (32, 32)
    fr = store.frames.cpu().numpy()
    out = prep.store_to_tensor(store, idx, out_hw=hw, flips=flips, offsets=offs).cpu()
    for n, f in enumerate(idx):
        a = np.copy(np.fliplr(fr[f])) if flips[n] else fr[f]
        a = a[offs[n][0]:offs[n][0] + hw[0], offs[n][1]:offs[n][1] + hw[1]]
        t, _ = CT.Compose([CT.ArrayToTensor(), CT.Normalize(prep.mean, prep.std)])([np.ascontiguousarray(a)], None)
        assert torch.equal(out[n], t[0]), n
    full = prep.store_to_tensor(store, [5]).cpu()
    t, _ = CT.Compose([CT.ArrayToTensor(), CT.Normalize(prep.mean, prep.std)])([fr[5]], None)
    assert torch.equal(full[0], t[0])
    # ids outside the store are refused before anything is launched: by the Python wrappers and by the entry points themselves
    for bad in ([0, 13], [-1], []):
        with pytest.raises(ValueError):
            prep.store_to_tensor(store, bad)
        with pytest.raises(ValueError):
            prep.store_resize_crop(store, bad, (40, 56), (36, 52))
    tr = CT.DeviceTrainTransform(device=dev)
    for bad in ([len(store)], [-1]):
        with pytest.raises(ValueError):
            tr.from_store(store, bad)
    from cc_amd._lib import engine, STREAM
    E = engine()
    ih = np.array([0, 13], dtype=np.int32)
    i_d = torch.zeros(2, dtype=torch.int32, device=dev)
    geo = torch.zeros(2, 8, dtype=torch.int32, device=dev)
    dst = torch.empty(2, 3, 36, 52, device=dev)
    u8 = torch.empty(2, 36, 52, 3, dtype=torch.uint8, device=dev)
    rot = torch.zeros(2, 8, dtype=torch.float64, device=dev)
    with pytest.raises(RuntimeError, match="code -1"):
        E.call("cc_store_to_tensor", store.frames, 13, ih.ctypes.data, i_d, dst, geo, 2, 36, 52, 36, 52, 0., 0., 0., 1., 1., 1., STREAM)
    with pytest.raises(RuntimeError, match="code -1"):
        E.call("cc_store_resize_to_tensor", store.frames, store.minmax, 13, ih.ctypes.data, i_d, dst, geo, geo, 2, u8, 2, 36, 52, 52, 52,
               36, 52, 0., 0., 0., 1., 1., 1., STREAM)
    with pytest.raises(RuntimeError, match="code -1"):
        E.call("cc_store_rotate", store.frames, store.minmax, 13, ih.ctypes.data, i_d, u8, rot, 2, 36, 52, STREAM)


# ----------------------------------------------------------------------------- 5. local normalisation
def check_local_norm(dev, tmp_root, sizes=((36, 52),)):
    """`normalize='local'` against the host NormalizeLocally in fp32 and the same arithmetic in float64, under the project's bar
    (tests/parity.py: e_dev <= 4 e_32 + 2^-23, e = max|x - f64| / max|f64|), B = 3 samples of nf = 3 and 5 frames."""
    from parity import _RigidTerms
    for (H, W) in sizes:
        for nf in (3, 5):
            root, store = tree_and_store(dev, tmp_root, H, W, nf)
            ids = [len(store) - 1, 2, 0] if nf == 5 else [5, 1, 6]     # both scenes; with and without the constant frame
            samples = host_samples(store, root, ids)
            h32 = host_pipeline(samples, True, [CT.NormalizeLocally()])
            raw = host_pipeline(samples, True, [])
            tr = CT.DeviceTrainTransform(device=dev, rotate=True, normalize="local")
            random.seed(11)
            np.random.seed(11)
            out, Ks = tr.from_store(store, ids)
            random.seed(11)
            np.random.seed(11)
            fm, _ = tr.from_store(store, ids, frame_major=True)
            assert torch.equal(fm.permute(1, 0, 2, 3, 4), out)                 # the same sums in the same order
            random.seed(11)
            np.random.seed(11)
            dense, _ = tr(samples)
            assert torch.equal(dense, out)
            terms = _RigidTerms("local_norm %dx%d nf=%d" % (H, W, nf))
            for b in range(len(ids)):
                x64 = torch.stack(raw[b][0]).double()                          # [nf,3,h,w], x / 255 exactly as the device holds it
                m = x64.transpose(0, 1).reshape(3, -1).mean(1).view(1, 3, 1, 1)
                s = x64.transpose(0, 1).reshape(3, -1).std(1).view(1, 3, 1, 1)   # unbiased, as NormalizeLocally takes it
                terms.term("sample %d" % b, out[b], torch.stack(h32[b][0]), (x64 - m) / s)
                assert np.array_equal(np.asarray(Ks[b]), np.asarray(h32[b][1]))
            terms.done()


# ----------------------------------------------------------------------------- 6. loader
def check_loader_order(store):
    S = len(store)
    assert S >= 9
    for world, B in ((1, 2), (3, 2), (3, 1)):
        loaders = [DS.DeviceSequenceLoader(store, B, None, seed=5, rank=r, world_size=world) for r in range(world)]
        for e in (0, 1):
            for ld in loaders:
                ld.set_epoch(e)
            perm = torch.randperm(S, generator=torch.Generator().manual_seed(5 + e)).numpy()
            cut = perm[:S // (world * B) * (world * B)]
            got = [ld.indices() for ld in loaders]
            assert all(len(ld) == len(cut) // (world * B) and len(g) == len(ld) * B for ld, g in zip(loaders, got))
            assert all(np.array_equal(g, cut[r::world]) for r, g in enumerate(got))
            assert len(set(np.concatenate(got).tolist())) == len(cut) and set(np.concatenate(got).tolist()) == set(cut.tolist())
        a = loaders[0].indices()
        loaders[0].set_epoch(0)
        assert not np.array_equal(a, loaders[0].indices())
    plain = DS.DeviceSequenceLoader(store, 2, None, shuffle=False)
    assert np.array_equal(plain.indices(), np.arange(S // 2 * 2))
    tail = DS.DeviceSequenceLoader(store, 4, None, shuffle=False, drop_last=False)
    assert len(tail) == -(-S // 4) and np.array_equal(tail.indices(), np.arange(S))


def check_loader_batches(dev, tmp_root, H, W, B=2, step=None, n_batches=3):
    """n_batches consecutive batches of the loader (5 samples: two batches per epoch, so the third is the next epoch's first)
    against the host pipeline under the same seeds -- pixels, K and Kinv exactly; step: called with each batch"""
    root, store = tree_and_store(dev, tmp_root, H, W)
    tr = CT.DeviceTrainTransform(MEAN, STD, device=dev, rotate=True)
    ld = DS.DeviceSequenceLoader(store, B, tr, seed=2)
    assert len(ld) == len(store) // B == 2
    epochs = -(-n_batches // len(ld))
    ids = []
    for e in range(epochs):
        ld.set_epoch(e)
        ids += ld.indices().tolist()
    host = host_pipeline(host_samples(store, root, ids[:n_batches * B]), True, [CT.Normalize(mean=MEAN, std=STD)])
    random.seed(11)
    np.random.seed(11)
    k = 0
    for e in range(epochs):
        ld.set_epoch(e)
        for tgt, refs, K, Kinv in ld:
            if k == n_batches:
                break
            assert tgt.shape == (B, 3, H, W) and len(refs) == 4 and K.shape == Kinv.shape == (B, 3, 3)
            for t in [tgt] + refs + [K, Kinv]:
                assert t.dtype == torch.float32 and t.is_contiguous() and t.device.type == torch.device(dev).type
            kept = [t.cpu() for t in [tgt] + refs + [K, Kinv]]
            if step is not None:
                step((tgt, refs, K, Kinv))
            for b in range(B):
                imgs, Kh = host[k * B + b]
                Kh = np.asarray(Kh, dtype=np.float32)
                assert np.array_equal(kept[5][b].numpy(), Kh) and np.array_equal(kept[6][b].numpy(), np.linalg.inv(Kh))
                for i, im in enumerate(imgs):
                    assert torch.equal(kept[i][b], im), (k, b, i)
            k += 1
    assert k == n_batches
