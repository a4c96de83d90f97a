"""A short KITTI 2015 evaluation at the protocol's sizes (networks at 256x832, ground truth at 375x1242) on a synthetic tree
with seeded networks, to be run under `rocprofv3 --kernel-trace --stats` (tools/gpu.sh step `flowprof`): evaluate_mask and
evaluate_flow over N samples, so that the kernel statistics hold k_png16_flow_decode, k_census_max, k_rigidity_compose_norm and
k_mask_iou_counts.  Also prints the host's zlib inflate time per ground-truth file (time.perf_counter), the other half of the
reader's cost.

    python tools/kitti_flow_profile.py [N]
"""
import os
import pathlib
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import test_kitti_flow_eval as T  # noqa: E402
from cc_amd import kitti_eval as K  # noqa: E402


def main(n):
    dev = torch.device("cuda")
    with tempfile.TemporaryDirectory() as tmp:
        tmp = pathlib.Path(tmp)
        T.make_kitti2015_tree(tmp, 375, 1242, n=n, seed=3)
        nets = T._nets(dev)
        for rep in range(2):                                            # the first pass warms the allocator and the plans up
            t0 = time.perf_counter()
            res = K.evaluate_mask(*nets, K.Kitti2015Flow(tmp, N=n, with_semantic=True))
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            err, names = K.evaluate_flow(*nets, K.Kitti2015Flow(tmp, N=n))
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            print("pass %d: evaluate_mask %.1f ms/sample, evaluate_flow %.1f ms/sample" % (rep, (t1 - t0) / n * 1e3, (t2 - t1) / n * 1e3))
        print("counts", res["counts"].tolist())
        print("flow errors", dict(zip(names, np.round(err, 4).tolist())))
        inflate, size = [], []
        for i in range(n):
            data = K.Kitti2015Flow(tmp, N=n).paths(i)["flow"].read_bytes()
            for _ in range(3):
                t0 = time.perf_counter()
                K.png16_scanlines(data)
                inflate.append(time.perf_counter() - t0)
            size.append(len(data))
        print("host: parse + zlib inflate + split of one 375x1242 flow PNG (%d KB compressed): median %.2f ms, min %.2f ms"
              % (np.mean(size) / 1024, np.median(inflate) * 1e3, np.min(inflate) * 1e3))
        # the decode alone, timed with events around 20 launches
        ftype, rows, W = K.png16_scanlines(data)
        ft, rw = torch.from_numpy(ftype).to(dev)[None], torch.from_numpy(rows).to(dev)[None]
        K.png16_flow_decode(ft, rw, W)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(20):
            K.png16_flow_decode(ft, rw, W)
        b.record()
        torch.cuda.synchronize()
        print("device: cc_png16_flow_decode of one file: %.3f ms (events around 20 launches)" % (a.elapsed_time(b) / 20))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 6)
