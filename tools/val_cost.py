"""What the two per-epoch validation passes cost, from the files and from the resident stores (cc_amd/datasets/validation.py).

Synthetic trees in a temporary directory, seeded networks, nothing read from outside:
  flow   a KITTI 2015 tree of N samples cycling through the data set's four ground-truth sizes, networks at 256 x 832
         (a) kitti_eval.evaluate_flow(framework): today's pass -- five PNGs decoded by Pillow, byte-scaled, the ground-truth PNG
             inflated, everything uploaded, per sample and per epoch
         (b) the same errors from a FlowValStore at batch size 1
         (c) from the store at batch size 8
  depth  a validation folder of F frames of 256 x 832 with a depth map each
         (a) validate_depth_with_gt over DataLoader(ValidationSet(...), batch_size 8, 4 persistent workers, pinned memory)
         (b) validate_depth_from_store at batch size 1
         (c) at batch size 8
Each path is warmed up once, then timed in three rounds that alternate (a), (b), (c); a timed region lies between two device events
after a full synchronise, ends in the pass's own host read-back, and the reported time is the median of the three rounds.  Building
the stores is timed once, apart.  Also reported: the largest relative difference of the eight flow errors between (c) and (b)
(batched forward passes may choose other convolution plans; reported, not asserted).

    python tools/val_cost.py [--samples 24] [--frames 96] [--out profiles/val_store_cost.txt]
"""
import argparse
import os
import statistics
import sys
import tempfile
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

KITTI_SIZES = ((375, 1242), (370, 1224), (374, 1238), (376, 1241))
HW = (256, 832)


def timed(fn):
    """-> (milliseconds between two device events around fn, fn's result); fn ends in its own host read-back"""
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def rounds(paths, n=3):
    """paths: [(name, fn)] -> {name: (median ms, [ms per round], last result)}; one warm-up each, then n alternating rounds"""
    last = {}
    for name, fn in paths:
        last[name] = fn()
    ms = {name: [] for name, _ in paths}
    for _ in range(n):
        for name, fn in paths:
            t, last[name] = timed(fn)
            ms[name].append(t)
    return {name: (statistics.median(v), v, last[name]) for name, v in ms.items()}


def build_depth_tree(root, frames):
    from PIL import Image
    r = np.random.RandomState(1)
    os.makedirs(os.path.join(root, "scene_0"))
    coarse = r.rand(HW[0] // 8, HW[1] // 8, 3)
    for i in range(frames):
        img = np.kron(np.roll(coarse, i, 1), np.ones((8, 8, 1))) * 200 + r.rand(HW[0], HW[1], 3) * 40
        Image.fromarray(img.astype(np.uint8), mode="RGB").save(os.path.join(root, "scene_0", "%07d.jpg" % i), quality=90)
        d = r.rand(*HW) * 90.0
        d[r.rand(*HW) < 0.5] = 0.0
        np.save(os.path.join(root, "scene_0", "%07d.npy" % i), d)
    with open(os.path.join(root, "val.txt"), "w") as f:
        f.write("scene_0\n")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--samples", type=int, default=24)
    p.add_argument("--frames", type=int, default=96)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "val_store_cost.txt"))
    a = p.parse_args()
    assert torch.cuda.is_available(), "val_cost.py measures on the GPU; there is no other path"
    import pathlib
    import validation_store_cases as C
    from cc_amd import custom_transforms as CT, datasets as DS, kitti_eval as K, validate as V
    dev = torch.device("cuda")
    nets = C.seeded_nets(dev)
    args = types.SimpleNamespace(THRESH=0.01, flownet="Back2Future", spatial_normalize=False)
    lines = ["validation passes: files against resident stores (tools/val_cost.py; median of 3 alternating rounds, device events)",
             "device: %s" % torch.cuda.get_device_name(0), ""]
    with tempfile.TemporaryDirectory() as tmp:
        # ---------------------------------------------------------------------------------------------------------- flow
        n = a.samples
        sizes = tuple(KITTI_SIZES[i % 4] for i in range(n))
        tree = pathlib.Path(tmp) / "kitti2015"
        C.make_flow_tree(tree, sizes)
        fw = K.Kitti2015Flow(tree, N=n)
        t0 = time.perf_counter()
        store = DS.FlowValStore.build(fw, HW, device=dev)
        torch.cuda.synchronize()
        build_s = time.perf_counter() - t0
        res = rounds([("a", lambda: K.evaluate_flow(*nets, fw, THRESH=0.01, img_hw=HW)[0]),
                      ("b", lambda: np.asarray(V.validate_flow_from_store(store, *nets, batch_size=1, args=args)[0])),
                      ("c", lambda: np.asarray(V.validate_flow_from_store(store, *nets, batch_size=8, args=args)[0]))])
        lines += ["flow: %d synthetic KITTI 2015 samples, ground truth %s, networks at %d x %d" % (n, " ".join("%dx%d" % s for s in KITTI_SIZES), HW[0], HW[1]),
                  "  store: %.1f MB resident, built once in %.2f s" % (store.nbytes / 1e6, build_s)]
        for key, what in (("a", "evaluate_flow(framework), from the files"), ("b", "store, batch size 1"), ("c", "store, batch size 8")):
            m, v, _ = res[key]
            lines.append("  (%s) %-42s %9.1f ms  %7.2f ms/sample  x200: %6.2f s   rounds %s"
                         % (key, what, m, m / n, m / n * 0.2, " ".join("%.1f" % t for t in v)))
        eb, ec, ea = res["b"][2], res["c"][2], res["a"][2]
        lines += ["  largest relative difference of the eight errors, (c) against (b): %.3e" % float(np.max(np.abs(ec - eb) / np.abs(eb))),
                  "  largest relative difference of the eight errors, (b) against (a): %.3e" % float(np.max(np.abs(eb - ea) / np.abs(ea))),
                  "  errors (b): " + " ".join("%.6f" % e for e in eb), ""]
        del store
        # --------------------------------------------------------------------------------------------------------- depth
        F = a.frames
        droot = os.path.join(tmp, "depth")
        os.makedirs(droot)
        build_depth_tree(droot, F)
        t0 = time.perf_counter()
        dstore = DS.DepthValStore.build(droot, device=dev, workers=8)
        torch.cuda.synchronize()
        build_s = time.perf_counter() - t0
        host = torch.utils.data.DataLoader(DS.ValidationSet(droot, CT.Compose([CT.ArrayToTensor(), CT.Normalize([0.5] * 3, [0.5] * 3)])),
                                           batch_size=8, shuffle=False, num_workers=4, pin_memory=True, persistent_workers=True,
                                           timeout=120)
        res = rounds([("a", lambda: V.validate_depth_with_gt(host, nets[0])[0]),
                      ("b", lambda: V.validate_depth_from_store(dstore, nets[0], 1)[0]),
                      ("c", lambda: V.validate_depth_from_store(dstore, nets[0], 8)[0])])
        lines += ["depth: %d frames of %d x %d with a depth map each" % (F, HW[0], HW[1]),
                  "  store: %.1f MB resident, built once in %.2f s" % (dstore.nbytes / 1e6, build_s)]
        for key, what in (("a", "DataLoader(ValidationSet), batch 8, 4 workers"), ("b", "store, batch size 1"), ("c", "store, batch size 8")):
            m, v, _ = res[key]
            lines.append("  (%s) %-46s %9.1f ms  %7.2f ms/frame   rounds %s" % (key, what, m, m / F, " ".join("%.1f" % t for t in v)))
        ea, ec = np.asarray(res["a"][2]), np.asarray(res["c"][2])
        lines.append("  largest relative difference of the six errors, (c) against (a): %.3e" % float(np.max(np.abs(ec - ea) / np.abs(ea))))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
