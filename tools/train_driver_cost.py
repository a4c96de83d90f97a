#!/usr/bin/env python
"""What the training driver's loop (cc_amd.train.train_epoch) costs per step beside the bare replayed step of bench.py.
  * B=4, 832x256, a synthetic FrameStore of 64 distinct samples (68 seeded frames, sliding windows of five), its sample list tiled so
    that one epoch is at least --steps steps; DeviceTrainTransform with RandomRotate (all four networks trained), the step of
    bench.py's configuration (StepConfig(), the ledger on at the driver's capacity for --print-freq).
  * one epoch = train_epoch() between two device events (the host draws, the table uploads, the batch launches, the copy into the
    graph's buffers, the replay, a drain every --print-freq steps), after an untimed epoch that captures the graph.
  * alternating with `bench.py --gpus 1 --steps S --warmup W` in a child process, --rounds rounds each.
  * the candidate causes of a gap apart: the loader alone (host clock per batch: draws + uploads + launch issue; device events per
    batch: its kernels), and drain() alone (host clock).
Prints one line per measurement and a JSON summary line; --out FILE also writes the table."""
import argparse
import json
import os
import random
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from cc_amd import datasets as DS, train as TR, trainer as T
from cc_amd.custom_transforms import DeviceTrainTransform


def synthetic_store(dev, H, W, distinct, steps, batch):
    rs = np.random.RandomState(0)
    F = distinct + 4
    coarse = rs.rand(F, (H + 7) // 8 + 1, (W + 7) // 8 + 1, 3)
    frames = np.empty((F, H, W, 3), dtype=np.uint8)
    for f in range(F):
        frames[f] = (40.0 + (np.kron(coarse[f], np.ones((8, 8, 1)))[:H, :W] * 0.8 + rs.rand(H, W, 3) * 0.2) * 170.0).astype(np.uint8)
    fr = torch.from_numpy(frames).to(dev)
    mm = torch.stack([fr.view(F, -1).min(1).values, fr.view(F, -1).max(1).values], 1).float().contiguous()
    samples = np.array([[i + 2, i, i + 1, i + 3, i + 4] for i in range(distinct)], dtype=np.int32)
    reps = -(-steps * batch // distinct)
    samples = np.tile(samples, (reps, 1))
    K = np.array([[[0.58 * W, 0, 0.49 * W], [0, 1.92 * H, 0.46 * H], [0, 0, 1]]], dtype=np.float32)
    return DS.FrameStore(fr, mm, K, samples, np.zeros(len(samples), dtype=np.int32), ["synthetic"])


def bench_ms(steps, warmup):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                         check=True, capture_output=True, text=True, cwd=ROOT).stdout
    line = [json.loads(l) for l in out.splitlines() if l.startswith("{")][-1]
    return float(line["ms_per_step"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--width", type=int, default=832)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--print-freq", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=100)
    ap.add_argument("--bench-warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "train_driver_cost.py times the loop on a HIP device"
    dev = torch.device("cuda:0")
    store = synthetic_store(dev, args.height, args.width, args.distinct, args.steps, args.batch)
    loader = DS.DeviceSequenceLoader(store, args.batch, DeviceTrainTransform(device=dev, rotate=True), seed=0)
    steps = len(loader)
    torch.manual_seed(0)
    tr = T.CCTrainer(T.build_nets(dev), T.StepConfig(ledger=TR.ledger_capacity(args.print_freq)), use_graph=True)

    def epoch(e):
        random.seed(e)
        np.random.seed(e)
        loader.set_epoch(e)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        done, loss = TR.train_epoch(tr, loader, steps, args.print_freq, None, e)
        e1.record()
        torch.cuda.synchronize()
        assert done == steps and np.isfinite(loss)
        return e0.elapsed_time(e1) / steps, (time.perf_counter() - t0) * 1e3 / steps

    epoch(0)                                    # captures the graph
    drv, host, bench = [], [], []
    for r in range(args.rounds):
        d, h = epoch(1 + r)
        drv.append(d)
        host.append(h)
        bench.append(bench_ms(args.bench_steps, args.bench_warmup))
        print("round %d: driver epoch %.3f ms/step (wall %.3f)   bench.py %.3f ms/step" % (r, d, h, bench[-1]), flush=True)

    # the parts apart: the loader alone, drain() alone
    loader.set_epoch(9)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    n = sum(1 for _ in loader)
    t1 = time.perf_counter()
    e1.record()
    torch.cuda.synchronize()
    loader_host, loader_dev = (t1 - t0) * 1e3 / n, e0.elapsed_time(e1) / n
    t0 = time.perf_counter()
    for _ in range(20):
        tr.ledger.drain()
    drain_ms = (time.perf_counter() - t0) * 1e3 / 20

    med = lambda v: sorted(v)[len(v) // 2]
    lines = [
        "training driver loop against the bare replayed step, B=%d %dx%d, %d steps per epoch from %d distinct samples, print_freq %d"
        % (args.batch, args.width, args.height, steps, args.distinct, args.print_freq),
        "  driver, train_epoch (device events)   median %.3f ms/step   rounds %s" % (med(drv), " ".join("%.3f" % v for v in drv)),
        "  driver, train_epoch (host clock)      median %.3f ms/step   rounds %s" % (med(host), " ".join("%.3f" % v for v in host)),
        "  bench.py --gpus 1 (%d steps)          median %.3f ms/step   rounds %s   spread %.3f"
        % (args.bench_steps, med(bench), " ".join("%.3f" % v for v in bench), max(bench) - min(bench)),
        "  gap (medians)                         %.3f ms/step" % (med(drv) - med(bench)),
        "  loader alone, per batch               host %.3f ms (draws, tables, uploads, launch issue)   device %.3f ms (its kernels)" % (loader_host, loader_dev),
        "  ledger.drain() alone                  %.3f ms per call = %.3f ms/step at print_freq %d" % (drain_ms, drain_ms / args.print_freq, args.print_freq),
    ]
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"driver_ms_per_step": [round(v, 3) for v in drv], "driver_wall_ms_per_step": [round(v, 3) for v in host],
                      "bench_ms_per_step": bench, "gap_ms": round(med(drv) - med(bench), 3), "bench_spread_ms": round(max(bench) - min(bench), 3),
                      "loader_host_ms": round(loader_host, 3), "loader_device_ms": round(loader_dev, 3), "drain_ms": round(drain_ms, 3),
                      "steps": steps}))


if __name__ == "__main__":
    main()
