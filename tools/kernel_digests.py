"""One SHA-256 per output tensor of the entry points behind the shared small-kernel pieces (adam_update.h, cc::block_tree,
radix_select.h): the Adam entries, the gradient guard, the parameter statistics, the validation metrics, the KITTI Eigen errors,
the normalised rigidity composition, the fixed-point warp backward and the spatial normalisation, on the inputs of the tests' case
modules.  Run it on two checkouts (this file copied into the older one) and diff the listings: equal lines are equal bits.

    python tools/kernel_digests.py cpu      the x86 emulation build of the kernel sources
    python tools/kernel_digests.py cuda     the product library on the device
"""
import contextlib
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np          # noqa: E402
import torch                # noqa: E402


def show(name, t):
    a = t.detach().cpu().contiguous().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)
    print("%s  %-44s %s %s" % (hashlib.sha256(a.tobytes()).hexdigest(), name, a.dtype, list(a.shape)))


def main(dev):
    import grad_guard_cases as G
    import kitti_eval_cases as KE
    import kitti_flow_cases as KF
    import ledger_cases as LC
    import optim_hyper_cases as C
    import test_metrics_kernels as TM
    from cc_amd import kitti_eval as K, loss_functions as LF, metrics as M, validate as V
    from cc_amd._lib import engine, STREAM
    from oracle.make_golden import rigidity_inputs

    def t(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    # Adam: cc_adam_step / _segment against _hyper / _segment_hyper (wd 0), three rows with and without weight decay, the guarded
    # entry with coef < 1 (row 0), coef == 1 and -- in the poisoned second step -- finite == 0 (rows 1, 2); three ticks each
    for n in (3 * 1024 + 7, 64):
        for name, old, new in C.old_against_new(n, dev):
            show("adam n=%d %s old" % (n, name), old)
            show("adam n=%d %s new" % (n, name), new)
    whole, ranges, _ = C.rows_and_bounds(dev)
    for k, a, b in zip("pmv", whole, ranges):
        show("adam rows hyper " + k, a)
        show("adam rows segment_hyper " + k, b)
    gs = G.grads(dev)
    mx = G.max_norms(gs[0])
    for case, seq in (("clean", gs), ("poisoned", gs[:1] + [G.poisoned(gs[1])] + gs[2:])):
        for s, st in enumerate(G.guarded_steps(dev, seq, mx)):
            for k in ("p", "m", "v", "guard"):
                show("guard %s step %d %s" % (case, s + 1, k), st[k])
    for n in G.NORM_SIZES:
        for spike in (False, True):
            show("grad_sumsq n=%d spike=%d guard row" % (n, spike), G.norm_case(n, dev, spike)[0])
    # parameter statistics (k_param_chunk / k_param_finish)
    for case in ("finite", "nonfinite"):
        _nets, opt = LC.bucket(dev)
        if case == "nonfinite":
            opt.flat_g[opt.offsets[5]] = LC.NAN
            opt.flat_g[opt.offsets[5] - 1] = LC.INF
        opt.param_stats(grad_scale=0.5, sync=True)
        show("param_stats %s partials" % case, opt._pstats["partials"])
        show("param_stats %s stats" % case, opt._pstats["stats"])
    # validation metrics (k_flow_metrics, the depth medians and terms)
    for B in (1, 3):
        gt, rigid, nonrigid, masks = [x.to(dev) if torch.is_tensor(x) else [m.to(dev) for m in x]
                                      for x in TM._flow_case(B, 47, 155, 32, 104, [(32, 104), (47, 155)], seed=5 + B)]
        show("flow_metrics B=%d two masks" % B, M.flow_metrics(gt, rigid, nonrigid, masks=masks, THRESH=0.5))
        show("flow_metrics B=%d one mask" % B, M.flow_metrics(gt, rigid, nonrigid, masks=masks[:1]))
        out, emap = M.flow_metrics(gt, rigid, epe_map=True)
        show("flow_metrics B=%d no mask" % B, out)
        show("flow_metrics B=%d epe map" % B, emap)
    dg, dp = [x.to(dev) for x in TM._depth_case()]
    for crop in (True, False):
        show("depth_errors crop=%d all" % crop, M.depth_errors(dg, dp, crop))
        for b in range(dg.shape[0]):
            show("depth_errors crop=%d sample %d" % (crop, b), M.depth_errors(dg[b:b + 1], dp[b:b + 1], crop))
    # KITTI Eigen errors (k_eigen_hist / _select / _terms), even and odd counts
    for seed, even in ((14, True), (15, False)):
        gt, pred, disp, norm = KE.eigen_case(seed, even=even)
        show("eigen_errors seed %d pose" % seed, K.eigen_errors(t(gt), t(pred), 1e-3, 80, t(disp), t(norm)))
        show("eigen_errors seed %d plain" % seed, K.eigen_errors(t(gt), t(pred), 1e-3, 80))
    # rigidity compositions (k_census_max + k_rigidity_compose_norm, k_rigidity_compose)
    r = K.rigidity_composition_norm(*[t(a) for a in KF.compose_inputs(24, 40, 53, B=2)], KF.THRESH)
    for k, v in sorted(vars(r).items()):
        show("compose_norm " + k, v)
    ri = rigidity_inputs()
    r = V.rigidity_composition(ri["explainability_mask"].to(dev), ri["flow_cam"].to(dev), ri["flow_fwd"].to(dev), ri["THRESH"])
    for k, v in sorted(vars(r).items()):
        show("compose " + k, v)
    # fixed-point warp backward (k_fx_absmax), the inputs of parity.check_feature_warp_deterministic
    E, g = engine(), torch.Generator().manual_seed(17)
    for (B, Cc, H, W) in ((2, 32, 16, 24), (1, 96, 12, 20), (2, 128, 8, 13)):
        feat = torch.randn(B, Cc, H, W, generator=g).to(dev)
        flow = (torch.randn(B, 2, H, W, generator=g) * 6.0).to(dev)
        gout = (torch.randn(B, Cc, H, W, generator=g) * 1e-4).to(dev)
        ws = torch.empty(int(E.call("cc_feature_warp_bwd_det_ws_bytes", B, Cc, H, W)), dtype=torch.uint8, device=dev)
        got, gflow = torch.empty_like(feat), torch.empty_like(flow)
        E.call("cc_feature_warp_bwd_det", gout, feat, flow, gflow, got, ws, B, Cc, H, W, 0, 0.625, 0, STREAM)
        show("warp_bwd_det %s gfeat" % ((B, Cc, H, W),), got)
        show("warp_bwd_det %s gflow" % ((B, Cc, H, W),), gflow)
    # spatial normalisation (cc::block_sum_f64), forward and backward over three levels
    g = torch.Generator().manual_seed(3)
    xs = [(torch.rand(2, 1, h, w, generator=g) + 0.05).to(dev).requires_grad_(True) for h, w in ((64, 104), (31, 53), (4, 7))]
    dns, dps = LF.normalized_depth_levels(xs)
    sum((a * a).sum() + b.sum() for a, b in zip(dns, dps)).backward()
    for k, (x, a, b) in enumerate(zip(xs, dns, dps)):
        show("spatial_norm level %d dn" % k, a)
        show("spatial_norm level %d depth" % k, b)
        show("spatial_norm level %d grad" % k, x.grad)


if __name__ == "__main__":
    dev = sys.argv[1] if len(sys.argv) > 1 else "cpu"
    assert dev in ("cpu", "cuda"), "usage: kernel_digests.py cpu|cuda"
    ctx = contextlib.nullcontext()
    if dev == "cpu":
        from hipemu.emu import emulated_engine
        ctx = emulated_engine()
    with ctx:
        main(dev)
        if dev == "cuda":
            torch.cuda.synchronize()
