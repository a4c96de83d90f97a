#!/usr/bin/env python
"""What the step ledger (StepConfig.ledger) costs the captured step, and how long FlatAdam.param_stats() takes.
  1. B=4, 832x256, one process, the step replayed from its hipGraph and timed with device events -- ledger off / on, alternating,
     ROUNDS rounds, medians (the trainers are built one after the other: the weight-image registry belongs to the one built last).
  2. the param_stats sweep at the four full-size networks: device events around CALLS back-to-back issues of its two entry points
     alone (arguments prepared beforehand), beside the algorithmic bytes (2 buckets x 4 bytes x elements) and the resulting GB/s;
     cc_grad_sumsq (the gradient guard's sweep, ONE bucket) over each network's segment the same way as the yardstick; the host's
     issue time of each loop (the lower bound of such an event interval); and FlatAdam.param_stats() as a user calls it.
Prints one line per measurement and a JSON summary line."""
import argparse
import gc
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from cc_amd import synthetic as syn, trainer as T
from cc_amd._lib import engine, STREAM
from tools.guard_cost import replay_ms


def trainer(dev, ledger):
    torch.manual_seed(0)
    tr = T.CCTrainer(T.build_nets(dev), T.StepConfig(ledger=ledger), use_graph=True)
    assert tr.pipeline == "per_network"
    return tr


def events_ms(fn, calls):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--width", type=int, default=832)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ledger_cost.py times the step on a HIP device"
    dev = torch.device("cuda:0")
    bc = syn.sample(args.batch, args.height, args.width, seed=1)
    batch = (bc[0].to(dev), [r.to(dev) for r in bc[1]], bc[2].to(dev), bc[3].to(dev))
    ms = {"off": [], "on": []}
    stats = None
    for r in range(args.rounds):
        for key, cap in (("off", None), ("on", 4096)):
            tr = trainer(dev, cap)
            ms[key].append(replay_ms(tr, batch, args.warmup, args.steps))
            if cap is not None:
                d = tr.ledger.drain()
                assert d.rows.shape[0] == args.warmup + args.steps and d.dropped == 0, (d.rows.shape, d.dropped)
            if key == "on" and r == args.rounds - 1:
                stats = param_stats_ms(tr, args.calls)
            del tr
            gc.collect()
            torch.cuda.empty_cache()
        print("round %d: ledger off %.3f  on %.3f ms/step" % (r, ms["off"][-1], ms["on"][-1]), flush=True)
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    print(json.dumps({"ms_per_step": {k: [round(x, 3) for x in v] for k, v in ms.items()},
                      "median": {k: round(v, 3) for k, v in med.items()}, "on_minus_off": round(med["on"] - med["off"], 3),
                      "spread": {k: round(max(v) - min(v), 3) for k, v in ms.items()},
                      "shape": [args.batch, args.height, args.width], "steps": args.steps, "rounds": args.rounds,
                      "param_stats": stats}))


def param_stats_ms(tr, calls):
    """Three figures per sweep, each from device events around `calls` back-to-back issues after a warm-up:
      *_launch_ms   the entry points alone, every argument prepared beforehand (tables, segment views): two launches per
                    param_stats, four per guard sweep -- as close to kernel time as events around asynchronous launches get (the
                    interval cannot be shorter than the host needs to issue them: `host_issue_ms`, the same loop timed with the
                    host clock, says how close to that bound it is);
      param_stats_call_ms   FlatAdam.param_stats() as a user calls it (sync=False)."""
    import time
    opt = tr.opt
    E = engine()
    n = opt.flat_p.numel()
    t = opt._param_stats_tables()
    nchunks, nparams, scale = int(t["chunks"].shape[0]), len(opt.params), float(opt.grad_scale())

    def stats_launches():
        E.call("cc_param_stats_chunks", opt.flat_g, opt.flat_p, n, t["chunks"], nchunks, t["partials"], STREAM)
        E.call("cc_param_stats_finish", t["partials"], t["first"], nparams, scale, t["stats"], STREAM)

    segs = [(opt.flat_g[a:b], b - a) for a, b in zip(opt.bounds, opt.bounds[1:]) if b > a]
    partials = torch.zeros(opt.GUARD_BLOCKS, device=opt.flat_p.device, dtype=torch.float64)

    def sumsq_launches():
        for view, k in segs:
            E.call("cc_grad_sumsq", view, k, partials, None, STREAM)

    def host_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        dt = (time.perf_counter() - t0) * 1e3 / calls        # (issue only: no synchronise inside the window)
        torch.cuda.synchronize()
        return dt

    out = {"elements": n, "parameters": nparams, "chunks": nchunks, "calls": calls,
           "param_stats_bytes": 2 * 4 * n, "grad_sumsq_bytes": 4 * n}
    out["param_stats_launch_ms"] = round(events_ms(stats_launches, calls), 4)
    out["param_stats_host_issue_ms"] = round(host_ms(stats_launches), 4)
    out["grad_sumsq_launch_ms"] = round(events_ms(sumsq_launches, calls), 4)
    out["grad_sumsq_host_issue_ms"] = round(host_ms(sumsq_launches), 4)
    out["param_stats_call_ms"] = round(events_ms(opt.param_stats, calls), 4)
    out["param_stats_call_host_issue_ms"] = round(host_ms(opt.param_stats), 4)
    out["param_stats_GBps"] = round(out["param_stats_bytes"] / out["param_stats_launch_ms"] * 1e-6, 1)
    out["grad_sumsq_GBps"] = round(out["grad_sumsq_bytes"] / out["grad_sumsq_launch_ms"] * 1e-6, 1)
    print("param_stats, entries alone: %(param_stats_launch_ms).4f ms (host issue %(param_stats_host_issue_ms).4f ms), %(param_stats_bytes)d "
          "bytes -> %(param_stats_GBps).1f GB/s (%(parameters)d parameters, %(chunks)d chunks); FlatAdam.param_stats(): "
          "%(param_stats_call_ms).4f ms (host issue %(param_stats_call_host_issue_ms).4f ms); cc_grad_sumsq over the four segments, entries "
          "alone: %(grad_sumsq_launch_ms).4f ms (host issue %(grad_sumsq_host_issue_ms).4f ms), %(grad_sumsq_bytes)d bytes -> "
          "%(grad_sumsq_GBps).1f GB/s" % out, flush=True)
    return out


if __name__ == "__main__":
    main()
