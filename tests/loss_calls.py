"""The loss phase of one training step (cc_amd.trainer.cc_forward + the losses' backward, bracketed as CCTrainer does) on seeded
stand-ins for the four networks' outputs, with a log of the engine calls it makes: names, every non-address argument, and the job
tables as (H, W, slots).  tests/golden/loss_calls.json pins that sequence for the 2 x 64 x 128 step (tests/test_step_emu.py);
`python tests/loss_calls.py` (x86 emulation build) rewrites it."""
import ctypes
import json
import os

import torch

from cc_amd import loss_functions as LF, synthetic as syn, trainer as T
from cc_amd._lib import engine, STREAM
from cc_amd.step_scope import StepScope
from oracle.make_golden import pyramid_inputs

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_calls.json")
LB, LH, LW = 2, 64, 128


class ArgLog:
    """tests/grad_guard_cases.py CallLog extended to the arguments: [name, [args]] per call.  An address is logged as "p" (0 when
    null), the stream not at all; a job table (first argument `jobs`) as njobs rows [H, W, [slots]], a slot being 0, "p" or the
    integer it carries (flags, channel counts); cc_scale_acc_jobs' table as rows [n floats, accumulate].  Subclasses choose the
    calls they keep (keeps) and how an argument is written down (arg): tests/conv_calls.py."""

    def __enter__(self):
        self.e, self.calls = engine(), []
        self.orig = self.e.call

        def call(name, *a):
            if self.keeps(name):
                types, names = self.e.sigs[name][1], self.e.sigs[name][2]
                self.calls.append([name, [self.arg(name, a, v, ty, an) for v, ty, an in zip(a, types, names)
                                          if not (an == "stream" or v is STREAM)]])
            return self.orig(name, *a)
        self.e.call = call
        return self

    def keeps(self, name):
        return True

    def arg(self, name, a, v, ty, an):
        if an == "jobs":
            tab = (ctypes.c_long * (10 * a[1])).from_address(v)
            return [[tab[10 * j + 8], tab[10 * j + 9], [self._slot(tab[10 * j + k]) for k in range(8)]] for j in range(a[1])]
        if an == "jobs_host":
            tab = (ctypes.c_long * (4 * a[1])).from_address(v)
            return [[tab[4 * j + 2], tab[4 * j + 3]] for j in range(a[1])]
        if ty is ctypes.c_void_p:
            return 0 if (v is None or (isinstance(v, int) and v == 0)) else "p"
        return v

    @staticmethod
    def _slot(v):
        return int(v) if abs(v) < (1 << 24) else "p"

    def __exit__(self, *a):
        del self.e.call
        return False


def loss_phase(dev, B=LB, H=LH, W=LW):
    """-> (losses {name: 0-dim tensor}, gradients of the network outputs, engine calls)"""
    tgt, refs, K, Kinv = syn.sample(B, H, W, seed=1, smooth=3)
    pyr = pyramid_inputs(B, H, W)
    pose = syn.kernel_inputs(B, 8, 8, seed=2)["pose"] * 0.1

    def leaves(key):
        return [p[key].clone().to(dev).requires_grad_(True) for p in pyr]
    disp, mask, ffw, fbw = leaves("depth"), leaves("mask"), leaves("flow_fwd"), leaves("flow_bwd")
    pose = pose.to(dev).requires_grad_(True)
    nets = (lambda t: disp, lambda t, r: pose, lambda t, r: mask, lambda t, r: (ffw, fbw, None))
    batch = (tgt.to(dev), [r.to(dev) for r in refs], K.to(dev), Kinv.to(dev))
    cut = {}
    try:
        with StepScope(batch[0].device) as scope, scope.loss_phase(), ArgLog() as log:
            out = T.cc_forward(nets, batch, T.StepConfig(), cut=cut)
            pairs = cut["dp"] + cut["mf"]
            grads = torch.autograd.grad(out["loss"], [d for _, d in pairs], allow_unused=True)
    finally:
        LF.pyramid_cache.clear()
        LF.take_nan_flags()
    losses = {k: v.detach().clone() for k, v in out.items() if torch.is_tensor(v) and k.startswith("loss")}
    return losses, [None if g is None else g.detach().clone() for g in grads], log.calls


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from hipemu.emu import emulated_engine
    with emulated_engine():
        calls = loss_phase("cpu")[2]
    with open(FIXTURE, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(c) for c in calls) + "\n]\n")
    print("wrote %s (%d calls)" % (FIXTURE, len(calls)))
