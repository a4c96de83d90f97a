"""A/B of FlowNetC6's 21 x 21 / dilation-2 cost volume: the gather kernels (cc_corr_patch_{fwd,bwd}) against the plane-GEMM kernels
(cc_corr_plane_{fwd,bwd}, csrc/corr_plane.hip) on the same inputs in ONE process, alternating through config.debug.corr_patch_gather.

    python tools/corr_patch_ab.py [--B 8 --C 256 --H 32 --W 104 --rounds 20 --warmup 5 --inner 4]

Forward and backward are timed separately with device events: every round times `inner` back-to-back calls of one path, then of the
other; the table gives the median per call over the rounds and their spread (min .. max).  In-map MACs (the (displacement, pixel)
pairs whose sample lies inside the map, x C x B; the backward pass computes both gradients: twice that) over the median time, and
the share of the fp32 matrix peak (157.3 TFLOP/s, 64 FLOP / clk / SIMD).  The times include the launch gaps of an eager stream;
kernel times proper come from a kernel trace of this script (`--rounds 3` is enough for that)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cc_amd import config, ops  # noqa: E402

PEAK_TFLOPS = 157.3
P, D = 21, 2


def in_map_pairs(H, W):
    off = (torch.arange(P) - (P - 1) // 2) * D
    ny = ((torch.arange(H)[None] + off[:, None] >= 0) & (torch.arange(H)[None] + off[:, None] < H)).sum()
    nx = ((torch.arange(W)[None] + off[:, None] >= 0) & (torch.arange(W)[None] + off[:, None] < W)).sum()
    return int(ny) * int(nx)


def main():
    ap = argparse.ArgumentParser()
    for k, v in (("B", 8), ("C", 256), ("H", 32), ("W", 104), ("rounds", 20), ("warmup", 5), ("inner", 4)):
        ap.add_argument("--" + k, type=int, default=v)
    a = ap.parse_args()
    assert a.rounds >= 1 and a.inner >= 1
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    f1 = torch.randn(a.B, a.C, a.H, a.W, generator=g).to(dev).requires_grad_(True)
    f2 = torch.randn(a.B, a.C, a.H, a.W, generator=g).to(dev).requires_grad_(True)
    gout = torch.randn(a.B, P * P, a.H, a.W, generator=g).to(dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.inner):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.inner

    times = {(p, m): [] for p in ("fwd", "bwd") for m in ("gather", "plane")}
    results = {}
    for rnd in range(a.warmup + a.rounds):
        for mode in ("gather", "plane"):
            config.debug.corr_patch_gather = mode == "gather"
            out = ops.correlate_patch(f1, f2, P, D)
            tf = timed(lambda: ops.correlate_patch(f1, f2, P, D))
            tb = timed(lambda: torch.autograd.grad(out, (f1, f2), gout, retain_graph=True))
            if rnd >= a.warmup:
                times[("fwd", mode)].append(tf)
                times[("bwd", mode)].append(tb)
            if rnd == 0:
                results[mode] = (out.detach().clone(),) + tuple(t.clone() for t in torch.autograd.grad(out, (f1, f2), gout))
    config.debug.corr_patch_gather = False
    same = [torch.equal(x, y) for x, y in zip(results["gather"], results["plane"])]
    pairs = in_map_pairs(a.H, a.W)
    macs = {"fwd": pairs * a.C * a.B, "bwd": 2 * pairs * a.C * a.B}
    print("corr_patch A/B  B %d C %d H %d W %d  P %d D %d  rounds %d x %d calls (warm-up %d)" % (a.B, a.C, a.H, a.W, P, D, a.rounds, a.inner, a.warmup))
    print("in-map share of the (displacement, pixel) pairs: %.1f %%; in-map MACs fwd %.3f G, bwd %.3f G" %
          (100.0 * pairs / (P * P * a.H * a.W), macs["fwd"] / 1e9, macs["bwd"] / 1e9))
    print("results equal bit for bit (out, g1, g2): %s" % same)
    print("%-4s %-7s %10s %10s %10s %12s %8s" % ("pass", "path", "median ms", "min ms", "max ms", "in-map TF/s", "of peak"))
    for p in ("fwd", "bwd"):
        for m in ("gather", "plane"):
            t = times[(p, m)]
            med = statistics.median(t)
            tf = 2.0 * macs[p] / (med * 1e-3) / 1e12
            print("%-4s %-7s %10.4f %10.4f %10.4f %12.2f %7.1f%%" % (p, m, med, min(t), max(t), tf, 100.0 * tf / PEAK_TFLOPS))
        tg, tp = times[(p, "gather")], times[(p, "plane")]
        spread = max(max(tg) - min(tg), max(tp) - min(tp))
        gain = statistics.median(tg) - statistics.median(tp)
        print("%-4s gather - plane = %.4f ms (x%.2f); larger spread of the two %.4f ms -> %s" %
              (p, gain, statistics.median(tg) / statistics.median(tp), spread, "faster" if gain > spread else "NOT faster by more than the spread"))


if __name__ == "__main__":
    main()
