"""Write tests/golden/recipe.npz: what the UNMODIFIED reference gives for the two recipe switches of train.py that the step takes --
`--spatial-normalize` (train.py:455-456) and `--no-non-rigid-mask` (train.py:483-488).  Arrays only.
Runs only where the reference tree exists (CC_REFERENCE_ROOT or the oracle's default); never in a test and never on a GPU machine.

Function level (keys `fn.<case>.<level>.*`): the reference's own loss_functions.spatial_normalize on the seeded inputs of
tests/recipe_cases.py -- `dn`, `depth` = 1 / dn (train.py:458) and `gx`, the gradient of sum(g_dn dn) + sum(g_depth depth) -- each
with the reference result's own largest distance from a float64 evaluation of the same formula as `<key>.ref_vs_f64` (relative for
the values; in units of recipe_cases.f64's `scale` for the gradient, whose terms cancel).

Step level (keys `<recipe>.*`, the keys oracle/make_golden.py net_and_step_level stores for the default recipe: six losses,
per-network gradient norms, small-parameter gradients, loss_after_adam), on its batch and seeded weights, through
oracle.step.cc_forward(impl = the reference):
  a  spatial_normalize: the reference DispResNet6 inside a module that returns [spatial_normalize(d) for d in net(x)] -- train.py:
     454-456, cc_forward takes depth = 1 / d next;
  b  no_non_rigid_mask: loss_4 recomputed from the run's kept flows with the reference's photometric_flow_loss(..., [None] * 6, ...),
     the total rebuilt from the five terms and backpropagated;
  c  both.

    python tools/make_recipe_golden.py [out.npz]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import recipe_cases as C  # noqa: E402
from cc_amd import synthetic as syn  # noqa: E402
from oracle import ref_import, step as S  # noqa: E402
from oracle.make_golden import SB, SH, SW, npy  # noqa: E402


def function_level(ref, g):
    lf = ref.loss_functions
    for name in C.NAMES:
        for l, (x, g_dn, g_dp) in enumerate(C.inputs(name)):
            xt = torch.from_numpy(x).requires_grad_(True)
            dn = lf.spatial_normalize(xt)
            depth = 1 / dn
            (gx,) = torch.autograd.grad((dn * torch.from_numpy(g_dn)).sum() + (depth * torch.from_numpy(g_dp)).sum(), [xt])
            want = C.f64(x, g_dn, g_dp)
            k = "fn.%s.%d." % (name, l)
            for key, got in (("dn", dn), ("depth", depth)):
                got = npy(got)
                g[k + key] = got
                g[k + key + ".ref_vs_f64"] = np.float64((np.abs(got - want[key]) / np.abs(want[key])).max())
            g[k + "gx"] = npy(gx)
            g[k + "gx.ref_vs_f64"] = np.float64((np.abs(npy(gx) - want["gx"]) / want["scale"]).max())


class Normalized(torch.nn.Module):
    """train.py:454-456: disparities = disp_net(tgt); disparities = [spatial_normalize(disp) for disp in disparities]"""

    def __init__(self, net, lf):
        super().__init__()
        self.net, self.lf = net, lf

    def forward(self, x):
        return [self.lf.spatial_normalize(d) for d in self.net(x)]


def step_level(ref, recipe, g):
    lf = ref.loss_functions
    batch = syn.sample(SB, SH, SW, seed=1)
    tgt, refs, K, Kinv = batch
    nets = S.build_nets("ref", ref)
    for n in nets:
        n.load_state_dict(syn.seeded_state_dict(n, 0))
        n.train()
    run_nets = [Normalized(nets[0], lf) if recipe in ("a", "c") else nets[0]] + nets[1:]
    cfg = S.StepConfig()

    def forward():
        out = S.cc_forward(run_nets, batch, cfg, impl=ref, keep=True)
        if recipe in ("b", "c"):
            out["loss_4"] = lf.photometric_flow_loss(tgt, refs[1:3], [out["flow_bwd"], out["flow_fwd"]], [None] * len(out["exp_mask"]),
                                                     lambda_oob=cfg.lambda_oob, qch=cfg.qch, wssim=cfg.wssim)
            out["loss"] = (cfg.w1 * out["loss_1"] + cfg.w2 * out["loss_2"] + cfg.w3 * out["loss_3"] + cfg.w4 * out["loss_4"]
                           + cfg.w5 * out["loss_5"])
        return out
    pre = recipe + "."
    out = forward()
    for k in ("loss", "loss_1", "loss_2", "loss_3", "loss_4", "loss_5"):
        g[pre + k] = npy(out[k])
    out["loss"].backward()
    for name, n in zip(("disp", "pose", "mask", "flow"), nets):
        sq = 0.0
        for pn, p in n.named_parameters():
            if p.grad is None:
                continue
            sq += float(p.grad.double().pow(2).sum())
            if p.numel() <= 64:
                g[pre + "grad.%s.%s" % (name, pn)] = npy(p.grad)
        g[pre + "gradnorm." + name] = np.float64(sq ** 0.5)
    S.make_optimizer(nets, cfg).step()
    g[pre + "loss_after_adam"] = npy(forward()["loss"])


def main(out):
    assert ref_import.reference_available(), "reference tree not present"
    torch.set_num_threads(1)             # run-to-run bit reproducibility of the fixture
    ref = ref_import.load(None)          # as the reference executes under this torch (the flavour of tests/golden/step_acF.npz)
    g = {}
    function_level(ref, g)
    for recipe in ("a", "b", "c"):
        step_level(ref, recipe, g)
        print("recipe %s: loss %.8f, after Adam %.8f" % (recipe, float(g[recipe + ".loss"]), float(g[recipe + ".loss_after_adam"])))
    np.savez_compressed(out, **g)
    print("wrote %s (%d arrays, %d bytes)" % (out, len(g), os.path.getsize(out)))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else C.FIXTURE)
