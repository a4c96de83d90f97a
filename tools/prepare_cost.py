"""Where the time of `cc_amd.datasets.prepare` goes, per frame, on the GPU: N synthetic 375 x 1242 RGB PNGs into 256 x 832 with a
pool of T host threads, stage by stage as `prepare` runs them (one chunk = one pinned upload):

    PNG decode (pool)  |  upload  |  resize kernels (device events)  |  velodyne depth  |  download  |  JPEG encode + write (pool)

and, beside it, the host-only path on the same files in the same pool: Pillow decode -> Image.resize(BILINEAR) -> JPEG write per
frame, which is what the reference's script does.  Times are wall-clock around work that ends in a device synchronise, except the
resize, which is taken from device events; every stage is warmed by one chunk first.  No threshold: the table says which stage
bounds the run.  Needs a HIP device: without one it fails.

    python tools/prepare_cost.py [--frames 512] [--threads 16] [--chunk 64] [--points 120000] [--out FILE]
"""
import argparse
import os
import shutil
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cc_amd.datasets import prepare as P  # noqa: E402
from cc_amd.kitti_eval import velo_depth  # noqa: E402

SRC, DST = (375, 1242), (256, 832)


def photo_like(seed):
    """a frame that compresses like a photograph (about half its raw size as PNG): smooth structure plus sensor-like noise"""
    r = np.random.RandomState(seed)
    H, W = SRC
    coarse = r.rand(H // 16 + 2, W // 16 + 2, 3)
    base = np.kron(coarse, np.ones((16, 16, 1)))[:H, :W]
    return np.clip(base * 200.0 + 20.0 + r.normal(0.0, 4.0, (H, W, 3)), 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--points", type=int, default=120000, help="velodyne points per frame")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "prepare_cost.py measures on a HIP device; none found"
    from PIL import Image
    dev = torch.device("cuda")
    N, C = a.frames, a.chunk
    work = tempfile.mkdtemp(prefix="prepare_cost_")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    try:
        src_dir, out_dir, host_dir = (os.path.join(work, n) for n in ("src", "out", "host"))
        for d in (src_dir, out_dir, host_dir):
            os.makedirs(d)
        paths = [os.path.join(src_dir, "%010d.png" % i) for i in range(N)]
        with ThreadPoolExecutor(max_workers=a.threads) as pool:
            list(pool.map(lambda i: Image.fromarray(photo_like(i)).save(paths[i], format="PNG"), range(N)))
            png_bytes = sum(os.path.getsize(p) for p in paths) / N
            H, W = SRC
            h, w = DST
            buf = torch.empty((C, H, W, 3), dtype=torch.uint8, pin_memory=True)
            back = torch.empty((C, h, w, 3), dtype=torch.uint8, pin_memory=True)
            r = np.random.RandomState(5)
            d = r.uniform(3.0, 80.0, a.points)
            u, v = r.uniform(-60, W + 60, a.points), r.uniform(-40, H + 40, a.points)
            pts = np.stack([d, -(u - 0.49 * W) / (0.58 * W) * d, -(v - 0.5 * H) / (1.92 * H) * d, np.ones(a.points)], 1).astype(np.float32)
            Pm = np.array([[0.58 * W * w / W, 0, 0.49 * w, 30.0], [0, 1.92 * H * h / H, 0.5 * h, 0.2], [0, 0, 1.0, 0.003]]) @ \
                np.array([[0, -1.0, 0, 0], [0, 0, -1.0, 0], [1.0, 0, 0, 0], [0, 0, 0, 1.0]])
            Pd = torch.from_numpy(np.ascontiguousarray(Pm)).to(dev)

            def decode(job):
                i, k = job
                buf.numpy()[k][...] = P.load_png_rgb8(paths[i])

            def encode(job):
                i, k = job
                Image.fromarray(back.numpy()[k]).save(os.path.join(out_dir, "%010d.jpg" % i))

            def host_only(i):
                with Image.open(paths[i]) as im:
                    Image.fromarray(np.asarray(im.resize((w, h), Image.BILINEAR))).save(os.path.join(host_dir, "%010d.jpg" % i))

            sec = {k: 0.0 for k in ("decode", "upload", "resize", "depth", "download", "encode")}
            sync = torch.cuda.current_stream().synchronize
            t_all = 0.0
            for lo, warm in [(0, True)] + [(lo, False) for lo in range(0, N, C)]:      # the first chunk twice: once as the warm-up
                ids = list(range(lo, min(N, lo + C)))
                n = len(ids)
                t0 = time.perf_counter()
                list(pool.map(decode, [(i, k) for k, i in enumerate(ids)]))
                t1 = time.perf_counter()
                src = buf[:n].to(dev, non_blocking=True)
                sync()
                t2 = time.perf_counter()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = P.resize_u8(src, h, w, h)
                e1.record()
                sync()
                t3 = time.perf_counter()
                for _ in ids:
                    velo_depth(torch.from_numpy(pts).to(dev), Pd, h, w).cpu()
                sync()
                t4 = time.perf_counter()
                back[:n].copy_(out, non_blocking=True)
                sync()
                t5 = time.perf_counter()
                list(pool.map(encode, [(i, k) for k, i in enumerate(ids)]))
                t6 = time.perf_counter()
                if warm:
                    continue
                for k, dt in zip(("decode", "upload", "depth", "download", "encode"), (t1 - t0, t2 - t1, t4 - t3, t5 - t4, t6 - t5)):
                    sec[k] += dt
                sec["resize"] += e0.elapsed_time(e1) * 1e-3
                t_all += t6 - t0
            list(pool.map(host_only, range(min(N, C))))                  # warm-up
            t0 = time.perf_counter()
            list(pool.map(host_only, range(N)))
            t_host = time.perf_counter() - t0
            t0 = time.perf_counter()
            list(pool.map(lambda i: P.load_png_rgb8(paths[i]), range(N)))
            t_dec = time.perf_counter() - t0

        say("prepare cost on %s: %d frames %d x %d -> %d x %d, %d host threads, chunks of %d, PNG %.0f KB / frame, %d velodyne points / frame"
            % (torch.cuda.get_device_name(0), N, H, W, h, w, a.threads, C, png_bytes / 1024, a.points))
        say("%-44s %12s %8s" % ("stage", "ms / frame", "share"))
        names = {"decode": "PNG decode (pool)", "upload": "upload (pinned, per chunk)", "resize": "resize kernels (device events)",
                 "depth": "velodyne depth (upload + kernel + download)", "download": "download", "encode": "JPEG encode + write (pool)"}
        total = sum(sec.values())
        for k in ("decode", "upload", "resize", "depth", "download", "encode"):
            say("%-44s %12.4f %7.1f%%" % (names[k], sec[k] / N * 1e3, 100.0 * sec[k] / total))
        say("%-44s %12.4f" % ("all stages, wall", t_all / N * 1e3))
        say("%-44s %12.4f" % ("host-only path (Pillow resize)", t_host / N * 1e3))
        say("%-44s %12.4f" % ("PNG decode alone, same pool", t_dec / N * 1e3))
        bound = max(sec, key=sec.get)
        say("the run is bound by: %s (%.1f%% of the staged time); resize moves %.2f MB / frame in %.4f ms"
            % (names[bound], 100.0 * sec[bound] / total, (H * W * 3 + 2 * H * w * 3 + h * w * 3) / 1e6, sec["resize"] / N * 1e3))
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
