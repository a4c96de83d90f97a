#!/usr/bin/env python
"""What the gradient guard (StepConfig.max_grad_norm) costs the captured step: B=4, 832x256, one process, the step replayed from its
hipGraph and timed with device events -- guard off / max_grad_norm = inf (norms + NaN skip) / clipping (every network held to half
the norm it just had), alternating, ROUNDS rounds, medians.  The weight-image registry (ops.packs) is one per process and belongs
to the trainer built last, so the trainers are built one after the other; "inf" and "clipping" are the SAME captured graph (the
bound is a value in the hyperparameter table).  Prints one line per measurement and a JSON summary line."""
import argparse
import gc
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from cc_amd import synthetic as syn, trainer as T


def replay_ms(tr, batch, warmup, steps):
    for _ in range(warmup):
        tr.step(batch)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        tr.step(batch)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def trainer(dev, max_grad_norm):
    torch.manual_seed(0)
    tr = T.CCTrainer(T.build_nets(dev), T.StepConfig(max_grad_norm=max_grad_norm), use_graph=True)
    assert tr.pipeline == "per_network"
    return tr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--width", type=int, default=832)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "guard_cost.py times the step on a HIP device"
    dev = torch.device("cuda:0")
    bc = syn.sample(args.batch, args.height, args.width, seed=1)
    batch = (bc[0].to(dev), [r.to(dev) for r in bc[1]], bc[2].to(dev), bc[3].to(dev))
    ms = {"off": [], "inf": [], "clip": []}
    for r in range(args.rounds):
        tr = trainer(dev, None)
        ms["off"].append(replay_ms(tr, batch, args.warmup, args.steps))
        del tr
        gc.collect()
        torch.cuda.empty_cache()
        tr = trainer(dev, float("inf"))
        ms["inf"].append(replay_ms(tr, batch, args.warmup, args.steps))
        st = tr.grad_stats(sync=True)
        for name, v in st.items():
            assert v["finite"] == 1.0 and v["skipped"] == 0.0, (name, v)
            tr.opt.set_hyper(name, max_grad_norm=0.5 * v["norm"])
        g = tr.graph
        ms["clip"].append(replay_ms(tr, batch, args.warmup, args.steps))
        assert tr.graph is g
        coef = {k: round(v["coef"], 3) for k, v in tr.grad_stats(sync=True).items()}
        del tr
        gc.collect()
        torch.cuda.empty_cache()
        print("round %d: off %.3f  inf %.3f  clip %.3f ms/step   (coef in the last clipped step: %s)"
              % (r, ms["off"][-1], ms["inf"][-1], ms["clip"][-1], coef), flush=True)
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    print(json.dumps({"ms_per_step": {k: [round(x, 3) for x in v] for k, v in ms.items()},
                      "median": {k: round(v, 3) for k, v in med.items()},
                      "inf_minus_off": round(med["inf"] - med["off"], 3), "clip_minus_off": round(med["clip"] - med["off"], 3),
                      "shape": [args.batch, args.height, args.width], "steps": args.steps, "rounds": args.rounds}))


if __name__ == "__main__":
    main()
