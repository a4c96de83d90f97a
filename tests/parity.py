"""Shared parity cases: the HIP engine (cc_amd, through the C ABI) against the oracle on identical seeded
inputs.  `dev` is "cuda" for the real library (-m gpu) or "cpu" for the x86 emulation build of the same
kernel sources (tests/hipemu).  Tolerances are the ones SURVEY.md section 8c / BASELINE.json state."""
import numpy as np
import pytest
import torch

from cc_amd import synthetic as syn, inverse_warp as IW, loss_functions as LF, ssim as SS
from cc_amd.step_scope import StepScope
from oracle import geometry as G, losses as L
from oracle.make_golden import pyramid_inputs


def to(dev, *ts):
    out = [t.to(dev) if torch.is_tensor(t) else [x.to(dev) for x in t] for t in ts]
    return out if len(out) > 1 else out[0]


def rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def frac_bad(a, b, atol=1e-5, rtol=1e-4):
    """fraction of elements outside |a-b| <= atol + rtol*|b| (robust to isolated bilinear-tap flips: the host CPU
    the oracle runs on may round a sampling coordinate to the other side of an integer than the GPU does)."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float(((a - b).abs() > atol + rtol * b.abs()).double().mean())


def leaf(t, dev):
    return t.detach().clone().to(dev).requires_grad_(True)


def check_warps(dev, B=2, H=24, W=40, smooth=0, atol=1e-5):
    """a8/a9/a10 + Back2Future.warp vs the oracle run on THIS host's CPU: forward 1e-5 abs, gradients 2e-5 rel
    (bit-exactness is checked against the reference's own outputs in check_warps_bit_exact_vs_golden)."""
    tgt, refs, K, Kinv = syn.sample(B, H, W, seed=1, smooth=smooth)
    ki = syn.kernel_inputs(B, H, W)
    pose = ki["pose"] * 3
    Kd, Kinvd = to(dev, K, Kinv)
    for ac in (False, True):
        for pad in ("zeros", "border"):
            d, p, im = leaf(ki["depth"][:, 0], dev), leaf(pose[:, 0], dev), leaf(refs[0], dev)
            d0, p0, im0 = leaf(ki["depth"][:, 0], "cpu"), leaf(pose[:, 0], "cpu"), leaf(refs[0], "cpu")
            # the kernel boundary is P = K.[R|t]: feed the oracle's P so coordinates can be compared bit-for-bit
            o = IW.inverse_warp(im, d, p, Kd, Kinvd, padding_mode=pad, align_corners=ac)
            r = G.inverse_warp(im0, d0, p0, K, Kinv, padding_mode=pad, align_corners=ac)
            go = torch.randn(r.shape, generator=torch.Generator().manual_seed(5))
            o.backward(go.to(dev))
            r.backward(go)
            assert frac_bad(o, r, atol) < 2e-3, (frac_bad(o, r, atol), float((o.detach().cpu() - r.detach()).abs().max()))
            assert frac_bad(d.grad, d0.grad, max(1e-6, atol * 0.1) * float(d0.grad.abs().max())) < 2e-3
            # d(out)/d(img) is the bilinear weight itself: a coordinate difference of atol px shows up as ~4*atol*|go|
            tol_im = 1e-5 if atol <= 1e-5 else 8 * atol
            assert frac_bad(im.grad, im0.grad, tol_im) < 2e-3, frac_bad(im.grad, im0.grad, tol_im)
            assert rel(p.grad, p0.grad) < 1e-2, rel(p.grad, p0.grad)
        d, p = leaf(ki["depth"][:, 0], dev), leaf(pose[:, 1], dev)
        d0, p0 = leaf(ki["depth"][:, 0], "cpu"), leaf(pose[:, 1], "cpu")
        f, f0 = IW.pose2flow(d, p, Kd, Kinvd), G.pose2flow(d0, p0, K, Kinv)
        assert float((f.detach().cpu() - f0.detach()).abs().max()) < 1e-3
        gf = torch.randn(f0.shape, generator=torch.Generator().manual_seed(6))
        g1 = torch.autograd.grad(f, [d, p], gf.to(dev))
        g0 = torch.autograd.grad(f0, [d0, p0], gf)
        assert rel(g1[0], g0[0]) < 1e-4 and rel(g1[1], g0[1]) < 1e-4
        fl, im = leaf(ki["flow_fwd"], dev), leaf(refs[1], dev)
        fl0, im0 = leaf(ki["flow_fwd"], "cpu"), leaf(refs[1], "cpu")
        o, r = IW.flow_warp(im, fl, align_corners=ac), G.flow_warp(im0, fl0, align_corners=ac)
        assert frac_bad(o, r, atol) < 2e-3
        go = torch.randn(r.shape, generator=torch.Generator().manual_seed(7))
        g1 = torch.autograd.grad(o, [im, fl], go.to(dev))
        g0 = torch.autograd.grad(r, [im0, fl0], go)
        assert frac_bad(g1[0], g0[0], (1e-5 if atol <= 1e-5 else 8 * atol)) < 2e-3 and frac_bad(g1[1], g0[1], (1e-4 if atol <= 1e-5 else 8 * atol)) < 2e-3
        for FC in (8, 18):          # 18 >= 16 channels: the channel-group parallel backward (4 groups of 5,5,5,3)
            ft = torch.randn(B, FC, H, W, generator=torch.Generator().manual_seed(8))
            fe, fe0 = leaf(ft, dev), leaf(ft, "cpu")
            o, r = IW.feature_warp(fe, fl, align_corners=ac), G.feature_warp(fe0, fl0, align_corners=ac)
            assert frac_bad(o, r, atol) < 2e-3
            go = torch.randn(r.shape, generator=torch.Generator().manual_seed(9))
            g1 = torch.autograd.grad(o, [fe, fl], go.to(dev))
            g0 = torch.autograd.grad(r, [fe0, fl0], go)
            assert frac_bad(g1[0], g0[0], (1e-5 if atol <= 1e-5 else 8 * atol)) < 2e-3 and frac_bad(g1[1], g0[1], (1e-4 if atol <= 1e-5 else 8 * atol)) < 2e-3


def check_ssim(dev, cases=((2, 40, 70, 0), (1, 64, 96, 3), (2, 8, 26, 0), (1, 33, 31, 1))):
    """a11: per-pixel 2e-4 abs (fp32 cancellation noise of the reference itself), mean 1e-5 rel."""
    for (B, H, W, smooth) in cases:
        fr = syn.frames(B, H, W, seed=3, n_frames=2, smooth=smooth)
        x, y = leaf(fr[0], dev), leaf(fr[1], dev)
        x0, y0 = leaf(fr[0], "cpu"), leaf(fr[1], "cpu")
        o, r = SS.ssim(x, y), L.ssim(x0, y0)
        assert float((o.detach().cpu() - r.detach()).abs().max()) < 2e-4
        assert abs(float(o.mean()) - float(r.mean())) < 1e-5 * abs(float(r.mean())) + 1e-7
        go = torch.randn(r.shape, generator=torch.Generator().manual_seed(4))
        g1 = torch.autograd.grad(o, [x, y], go.to(dev))
        g0 = torch.autograd.grad(r, [x0, y0], go)
        assert rel(g1[0], g0[0]) < 5e-5 and rel(g1[1], g0[1]) < 5e-5
    xx = torch.rand(1, 3, 20, 30)
    assert float((SS.ssim(xx.to(dev), xx.to(dev)).cpu() - 1).abs().max()) < 1e-5     # ssim(x, x) == 1
    # the reference's ssim() takes any channel count and window size (ssim.py:42-76; the module form defaults to 11 taps): other
    # channel counts run on the same 13-tap kernels, other windows on the generic depth-wise path
    gen = torch.Generator().manual_seed(6)
    for C, win in ((1, 13), (4, 13), (2, 11), (3, 7)):
        a0, b0 = torch.rand(2, C, 24, 36, generator=gen), torch.rand(2, C, 24, 36, generator=gen)
        a1, b1 = leaf(a0, dev), leaf(b0, dev)
        a0, b0 = leaf(a0, "cpu"), leaf(b0, "cpu")
        o = SS.ssim(a1, b1, win) if win != 11 else SS.SSIM()(a1, b1)
        r = SS._ssim_generic(a0, b0, win)                                         # the reference's formula on the CPU
        assert o.shape == r.shape and float((o.detach().cpu() - r.detach()).abs().max()) < 2e-4, (C, win)
        go = torch.randn(r.shape, generator=gen)
        g1 = torch.autograd.grad(o, [a1, b1], go.to(dev))
        g0 = torch.autograd.grad(r, [a0, b0], go)
        assert rel(g1[0], g0[0]) < 5e-5 and rel(g1[1], g0[1]) < 5e-5, (C, win)


def _pyr(dev, B, H, W, smooth=0):
    tgt, refs, K, Kinv = syn.sample(B, H, W, seed=1, smooth=smooth)
    pyr = pyramid_inputs(B, H, W)
    pose = syn.kernel_inputs(B, 8, 8, seed=2)["pose"] * 3.0

    def mk(d):
        return dict(depth=[leaf(p["depth"], d) for p in pyr], mask=[leaf(p["mask"], d) for p in pyr],
                    ff=[leaf(p["flow_fwd"], d) for p in pyr], fb=[leaf(p["flow_bwd"], d) for p in pyr],
                    pose=leaf(pose, d), tgt=tgt.to(d), refs=[r.to(d) for r in refs], K=K.to(d), Kinv=Kinv.to(d))
    return mk(dev), mk("cpu")


def _cmp(name, l1, l0, w1, w0, ltol=1e-4, gtol=1e-4):
    assert abs(float(l1) - float(l0)) <= ltol * abs(float(l0)), (name, float(l1), float(l0))
    g1 = torch.autograd.grad(l1, w1, allow_unused=True)
    g0 = torch.autograd.grad(l0, w0, allow_unused=True)
    for a, b in zip(g1, g0):
        assert (a is None) == (b is None), name
        if b is not None:
            # max-norm where the two sides are arithmetic-identical, flip-tolerant otherwise (see frac_bad)
            # pose gradients are pixel sums over every (possibly flipped) tap: small tensors, 1e-2 of their max
            ok = rel(a, b) < gtol or (b.numel() < 1000 and _note("cmp:small_grad_rel", rel(a, b)) < 5e-3) or (
                frac_bad(a, b, gtol * float(b.abs().max()), 1e-3) < 2e-3 and
                float((a.detach().cpu() - b.detach()).norm() / (b.detach().norm() + 1e-30)) < 5e-2)
            assert ok, (name, rel(a, b))


def check_losses(dev, B=2, H=64, W=96, smooth=0):
    """a12-a17 with gradients (north-star bar: losses within 1e-4 rel of the reference CPU path)."""
    for ac in (False, True):
        a, o = _pyr(dev, B, H, W, smooth)
        _cmp("photometric_reconstruction_loss",
             LF.photometric_reconstruction_loss(a["tgt"], a["refs"], a["K"], a["Kinv"], a["depth"], a["mask"], a["pose"],
                                                wssim=0.997, qch=0.5, align_corners=ac),
             L.photometric_reconstruction_loss(o["tgt"], o["refs"], o["K"], o["Kinv"], o["depth"], o["mask"], o["pose"],
                                               wssim=0.997, qch=0.5, align_corners=ac),
             a["depth"] + a["mask"] + [a["pose"]], o["depth"] + o["mask"] + [o["pose"]])
        a, o = _pyr(dev, B, H, W, smooth)
        _cmp("photometric_reconstruction_loss(no mask, lambda_oob, qch=0.4)",
             LF.photometric_reconstruction_loss(a["tgt"], a["refs"], a["K"], a["Kinv"], a["depth"], [None] * 6, a["pose"],
                                                wssim=0.5, qch=0.4, lambda_oob=0.3, align_corners=ac),
             L.photometric_reconstruction_loss(o["tgt"], o["refs"], o["K"], o["Kinv"], o["depth"], [None] * 6, o["pose"],
                                               wssim=0.5, qch=0.4, lambda_oob=0.3, align_corners=ac),
             a["depth"] + [a["pose"]], o["depth"] + [o["pose"]])
        a, o = _pyr(dev, B, H, W, smooth)
        _cmp("photometric_flow_loss",
             LF.photometric_flow_loss(a["tgt"], a["refs"][1:3], [a["fb"], a["ff"]], [1 - m[:, 1:3] for m in a["mask"]],
                                      wssim=0.997, align_corners=ac),
             L.photometric_flow_loss(o["tgt"], o["refs"][1:3], [o["fb"], o["ff"]], [1 - m[:, 1:3] for m in o["mask"]],
                                     wssim=0.997, align_corners=ac),
             a["ff"] + a["fb"] + a["mask"], o["ff"] + o["fb"] + o["mask"])
    a, o = _pyr(dev, B, H, W, smooth)
    _cmp("explainability_loss", LF.explainability_loss(a["mask"]), L.explainability_loss(o["mask"]), a["mask"], o["mask"])
    for nm in ("depth", "ff", "mask"):
        a, o = _pyr(dev, B, H, W, smooth)
        # 5 scales: the 6th (2x3) makes the reference's smooth_loss NaN (mean over an empty tensor)
        _cmp("smooth_loss " + nm, LF.smooth_loss(a[nm][:5]), L.smooth_loss(o[nm][:5]), a[nm][:5], o[nm][:5])
        assert torch.isnan(LF.smooth_loss(a[nm])) and torch.isnan(L.smooth_loss(o[nm]))
        _cmp("edge_aware_smoothness_loss " + nm, LF.edge_aware_smoothness_loss(a["tgt"], a[nm]),
             L.edge_aware_smoothness_loss(o["tgt"], o[nm]), a[nm], o[nm])
    # the four smoothness terms of the training step as ONE job table (engine extension, cc_amd.trainer.cc_forward)
    a, o = _pyr(dev, B, H, W, smooth)
    _cmp("edge_aware_smoothness_sum", LF.edge_aware_smoothness_sum(a["tgt"], [a["depth"], a["ff"], a["fb"], a["mask"]]),
         sum(L.edge_aware_smoothness_loss(o["tgt"], o[nm]) for nm in ("depth", "ff", "fb", "mask")),
         a["depth"] + a["ff"] + a["fb"] + a["mask"], o["depth"] + o["ff"] + o["fb"] + o["mask"])
    a, o = _pyr(dev, B, H, W, smooth)
    with torch.no_grad():
        cf1 = [IW.pose2flow(d[:, 0], a["pose"][:, 2], a["K"], a["Kinv"]) for d in a["depth"]]
        cb1 = [IW.pose2flow(d[:, 0], a["pose"][:, 1], a["K"], a["Kinv"]) for d in a["depth"]]
        cf0 = [G.pose2flow(d[:, 0], o["pose"][:, 2], o["K"], o["Kinv"]) for d in o["depth"]]
        cb0 = [G.pose2flow(d[:, 0], o["pose"][:, 1], o["K"], o["Kinv"]) for d in o["depth"]]
        t1 = LF.consensus_exp_masks(cf1, cb1, a["ff"], a["fb"], a["tgt"], a["refs"][2], a["refs"][1], wssim=0.997, wrig=1.0)
        t0 = L.consensus_exp_masks(cf0, cb0, o["ff"], o["fb"], o["tgt"], o["refs"][2], o["refs"][1], wssim=0.997, wrig=1.0)
        for x, y in zip(t1, t0):
            assert float((x.cpu() != y).float().mean()) <= 2e-3      # discontinuous output: flip rate
        assert 0.2 < float(t0[0].mean()) < 0.95                        # both classes present at the fine level
        occ1 = LF.depth_occlusion_masks(a["depth"][0], a["pose"], a["K"], a["Kinv"])
        occ0 = L.depth_occlusion_masks(o["depth"][0], o["pose"], o["K"], o["Kinv"])
        assert float((occ1.cpu() != occ0).float().mean()) <= 1e-5
        big_b, big_f = o["fb"][0] * 3 + 4, o["ff"][0] * 3 + 4         # force occlusions (signed-sum rule, Q5)
        ob1, of1 = LF.occlusion_masks(big_b.to(dev), big_f.to(dev))
        ob0, of0 = L.occlusion_masks(big_b, big_f)
        assert torch.equal(ob1.cpu(), ob0) and torch.equal(of1.cpu(), of0) and 0.05 < float(ob0.mean()) < 0.95
        rf = [(x - y).abs() for x, y in zip(cf0, o["ff"])]
        rb = [(x - y).abs() for x, y in zip(cb0, o["fb"])]
    _cmp("consensus_depth_flow_mask",
         LF.consensus_depth_flow_mask(a["mask"], to(dev, rb), to(dev, rf), to(dev, t0), to(dev, t0), THRESH=0.5, wbce=0.5),
         L.consensus_depth_flow_mask(o["mask"], rb, rf, t0, t0, THRESH=0.5, wbce=0.5), a["mask"], o["mask"])


def check_occluded_photo_loss(dev, B=2, H=32, W=48):
    """photometric_flow_loss with flows large enough that the occlusion factor (1 - occ) is exercised."""
    tgt, refs, K, Kinv = syn.sample(B, H, W, seed=4)
    ki = syn.kernel_inputs(B, H, W, seed=9)
    fb, ff = ki["flow_bwd"] * 0.5 + 0.3, ki["flow_fwd"] * 0.5 + 0.3
    assert 0.05 < float(L.occlusion_masks(fb, ff)[0].mean()) < 0.95
    m = ki["mask"][:, :2].contiguous()
    a = dict(fb=leaf(fb, dev), ff=leaf(ff, dev), m=leaf(m, dev))
    o = dict(fb=leaf(fb, "cpu"), ff=leaf(ff, "cpu"), m=leaf(m, "cpu"))
    _cmp("photometric_flow_loss (occluded, single scale)",
         LF.photometric_flow_loss(tgt.to(dev), to(dev, refs[1:3]), [a["fb"], a["ff"]], a["m"], wssim=0.5),
         L.photometric_flow_loss(tgt, refs[1:3], [o["fb"], o["ff"]], o["m"], wssim=0.5),
         [a["fb"], a["ff"], a["m"]], [o["fb"], o["ff"], o["m"]])


def check_pyramid(dev):
    from cc_amd._lib import engine, STREAM
    x = syn.frames(2, 64, 96, seed=11, n_frames=1)[0]
    xd = x.to(dev)
    for (h, w) in ((32, 48), (16, 24), (2, 3), (20, 31)):
        ref = torch.nn.functional.adaptive_avg_pool2d(x, (h, w))
        out = torch.empty(2, 3, h, w, device=dev)
        engine().call("cc_adaptive_avg_pool", xd, out, 6, 64, 96, h, w, STREAM)
        assert float((out.cpu() - ref).abs().max()) < 1e-6
    packed = torch.empty(6 * (32 * 48 + 16 * 24 + 8 * 12 + 4 * 6 + 2 * 3), device=dev)
    engine().call("cc_pyramid_build", xd, packed, 6, 6, 64, 96, STREAM)      # one launch: all levels of each 32x32 tile
    off = 0
    for l in (1, 2, 3, 4, 5):
        h, w = 64 >> l, 96 >> l
        lv = packed[off:off + 6 * h * w].view(2, 3, h, w).cpu()
        assert float((lv - torch.nn.functional.adaptive_avg_pool2d(x, (h, w))).abs().max()) < 1e-6
        off += 6 * h * w
    # the frames of a step in ONE launch (loss_functions.pyramid_cache.prefetch -> cc_pyramid_build_multi): bit-identical to the
    # per-image launch, and what get() then returns
    from cc_amd import loss_functions as LF
    frames = [f.to(dev) for f in syn.frames(2, 64, 96, seed=12, n_frames=3)]
    LF.pyramid_cache.clear()
    LF.pyramid_cache.prefetch(frames)
    for f in frames:
        single = torch.empty_like(packed)
        engine().call("cc_pyramid_build", f, single, 6, 6, 64, 96, STREAM)
        off = 0
        for l in (1, 2, 3, 4, 5):
            h, w = 64 >> l, 96 >> l
            assert (h, w) in LF.pyramid_cache.items[id(f)][2], "prefetch did not fill the cache"
            assert torch.equal(LF.pyramid_cache.get(f, h, w), single[off:off + 6 * h * w].view(2, 3, h, w))
            off += 6 * h * w
    LF.pyramid_cache.clear()


def check_warps_bit_exact_vs_golden(dev, golden_dir):
    """Index arithmetic + blend of the warp kernels reproduce the REFERENCE's outputs bit-for-bit (fixtures written by
    the unmodified reference in the build container, oracle/make_golden.py) when given the reference's P = K.[R|t]
    (the kernel boundary).  Host-CPU independent: nothing is recomputed on this box's CPU."""
    import os
    from oracle.make_golden import FB, FH, FW
    tgt, refs, K, Kinv = syn.sample(FB, FH, FW, seed=1)
    pyr = pyramid_inputs(FB, FH, FW)
    d0 = pyr[0]["depth"][:, 0].to(dev)
    out = {}
    for tag, ac in (("acF", 0), ("acT", 1)):
        g = dict(np.load(os.path.join(golden_dir, "functions_%s.npz" % tag)))
        P = torch.from_numpy(g["P"]).reshape(-1, 12).to(dev)
        w = IW._InverseWarpFn.apply(refs[0].to(dev), d0, P, Kinv.to(dev), 0, ac).cpu().numpy()
        f = IW._Pose2FlowFn.apply(d0, P, Kinv.to(dev), 0).cpu().numpy()
        fw = IW.flow_warp(refs[1].to(dev), pyr[0]["flow_fwd"].to(dev), align_corners=bool(ac)).cpu().numpy()
        feat = syn.frames(FB, 16, 24, seed=7, n_frames=1)[0]
        feat = torch.cat([feat, feat.flip(1), feat * 0.5], 1)[:, :8].contiguous()
        flo = syn.kernel_inputs(FB, 16, 24, seed=8)["flow_fwd"]
        ft = IW.feature_warp(feat.to(dev), flo.to(dev), align_corners=bool(ac)).cpu().numpy()
        # the stand-alone halves (inverse_warp.py:31-79): pixel2cam -> cam2pixel with the reference's P reproduce its grid
        P34 = torch.from_numpy(g["P"]).to(dev)
        grid = IW.cam2pixel(IW.pixel2cam(d0, Kinv.to(dev)), P34[:, :, :3].contiguous(), P34[:, :, 3:].contiguous(), "zeros")
        # tap-flip rate: how many pixels sample a different 2x2 neighbourhood when P comes from THIS device's sin/cos
        # (cc_pose_proj_fwd) instead of the reference's CPU matrices -- the number behind the flip-tolerant gradient bars
        pose = syn.kernel_inputs(FB, 8, 8, seed=2)["pose"] * 3.0
        P_dev = IW.projection_matrix(pose[:, 0].to(dev), K.to(dev)).reshape(-1, 3, 4)
        grid_dev = IW.cam2pixel(IW.pixel2cam(d0, Kinv.to(dev)), P_dev[:, :, :3].contiguous(), P_dev[:, :, 3:].contiguous(), "zeros")

        def taps(gr):
            x = torch.floor((gr[..., 0] + 1) * (FW / 2.0) - 0.5) if not ac else torch.floor((gr[..., 0] + 1) / 2 * (FW - 1))
            y = torch.floor((gr[..., 1] + 1) * (FH / 2.0) - 0.5) if not ac else torch.floor((gr[..., 1] + 1) / 2 * (FH - 1))
            return x, y
        (xa, ya), (xb, yb) = taps(grid), taps(grid_dev)
        out[tag] = dict(inverse_warp=float(np.mean(w == g["inverse_warp"])), pose2flow=float(np.mean(f == g["pose2flow"])),
                        flow_warp=float(np.mean(fw == g["flow_warp"])), feature_warp=float(np.mean(ft == g["feature_warp"])),
                        grid=float(np.mean(grid.cpu().numpy() == g["grid_zeros"])),
                        tap_flip_rate_device_P=float(((xa != xb) | (ya != yb)).float().mean()),
                        P_max_rel_diff=float((P_dev - P34).abs().max() / P34.abs().max()),
                        maxabs=float(np.abs(w - g["inverse_warp"]).max()))
    return out


MEASURED = {}      # worst value seen per bar (printed by the tests: the bars below are held at ~2x what is measured)


def _note(key, v):
    MEASURED[key] = max(MEASURED.get(key, 0.0), float(v))
    return v


def _grad_ok(gr, ref, tight):
    """tight: max-norm 2e-4 of the gradient's max.  Otherwise (white-noise frames, where the last-ulp difference
    between this device's P = K.[R|t] and the reference's can move a bilinear tap across a pixel boundary):
    all but 5e-4 of the elements within 1e-4 of the max, and 5e-3 in L2 (the elements that ARE off are pinned to tap
    boundaries by _flip_pinned)."""
    mx = float(ref.abs().max())
    l2 = float((gr.detach().cpu() - ref).norm() / (ref.norm() + 1e-30))
    if tight:
        # low-pass frames: a flipped tap changes the interpolation SLOPE at that pixel only slightly -> 5e-3 in L2
        return rel(gr, ref) < 2e-4 or (ref.numel() < 1000 and rel(gr, ref) < 2e-3) or \
            (frac_bad(gr, ref, 1e-4 * mx, 1e-3) < 2e-3 and l2 < 5e-3)
    if ref.numel() < 1000:          # pose gradient: a pixel sum over every (possibly flipped) tap (measured worst 2.5e-3)
        return _note("noise:pose_grad_rel", rel(gr, ref)) < 5e-3
    if rel(gr, ref) < 2e-4:
        return True
    # measured (emulator and MI355X): 1.6e-4 of the elements off the tight bar, 1.5e-3 in L2 -> bars at ~3x that
    return _note("noise:frac_bad", frac_bad(gr, ref, 1e-4 * mx, 1e-3)) < 5e-4 and _note("noise:l2", l2) < 5e-3


def _tap_boundary_distance(a, i, ac):
    """Distance (pixels) of every rigid sampling coordinate of pyramid level i to the nearest bilinear tap boundary (an
    integer coordinate), minimum over the four reference frames -- from the ORACLE's P on the host (loss_functions.py:91-92
    intrinsics scaling, inverse_warp.py:66-72 normalisation, ATen's grid_sampler unnormalise).  -> [B,H,W]"""
    d = a["depth"][i].detach().cpu()[:, 0]
    B, h, w = d.shape
    down = a["tgt"].shape[2] / h
    K, Kinv = a["K"].detach().cpu(), a["Kinv"].detach().cpu()
    K_s = torch.cat((K[:, 0:2] / down, K[:, 2:]), dim=1)
    Kinv_s = torch.cat((Kinv[:, :, 0:2] * down, Kinv[:, :, 2:]), dim=2)
    best = torch.full((B, h, w), 1.0)
    for r in range(a["pose"].shape[1]):
        grid = G.warp_grid(d, a["pose"].detach().cpu()[:, r], K_s, Kinv_s, padding_mode=None)
        for c, n in ((0, w), (1, h)):
            pix = (grid[..., c] + 1) / 2 * (n - 1) if ac else ((grid[..., c] + 1) * n - 1) / 2
            best = torch.minimum(best, (pix - pix.round()).abs())
    return best


def _flip_pinned(name, a, wrt_keys, grads, g, ac):
    """White-noise frames, rigid warp: the product computes P = K.[R|t] with its own sin/cos (cc_pose_proj_fwd), one ulp away
    from the reference's; where a sampling coordinate sits within ~1e-4 px of an integer the bilinear taps -- and, on noise,
    that pixel's gradient -- change.  This pins that mechanism: EVERY depth-gradient element outside 1e-4 of the maximum lies
    at a pixel whose coordinate is within 2e-3 px of a tap boundary, there are only a handful of them, and everything else
    meets the tight bar.  -> number of such elements."""
    nflip = 0
    for k, gr in zip(wrt_keys, grads):
        if gr is None or not k.startswith("depth"):
            continue
        ref = torch.from_numpy(g[name + ".grad." + k])
        bad = (gr.detach().cpu() - ref).abs() > 1e-4 * float(ref.abs().max())
        if bool(bad.any()):
            near = _tap_boundary_distance(a, int(k[5:]), ac) < 2e-3
            assert bool((near.unsqueeze(1) | ~bad).all()), (name, k, "a gradient element off the tight bar is NOT at a tap boundary")
            nflip += int(bad.sum())
            assert int(bad.sum()) <= max(4, ref.numel() // 2000), (name, k, int(bad.sum()))
    return nflip


def check_losses_vs_golden(dev, golden_dir, values=None):
    """a12-a17 (+ gradients) against the fixtures the UNMODIFIED reference wrote (oracle/make_golden.py): the
    host-CPU-independent parity gate.  Losses within 1e-4 rel (north star) on white-noise AND low-pass frames;
    gradients: tight on the low-pass frames, flip-tolerant on white noise (see _grad_ok).
    values: a dict that receives {case: (loss, {input: gradient})} of every checked call."""
    import os
    from oracle.make_golden import FB, FH, FW
    res = {}
    values = {} if values is None else values
    for tag, ac in (("acF", False), ("acT", True)):
        for smooth, suffix in ((0, ""), (3, "_smooth")):
            g = dict(np.load(os.path.join(golden_dir, "functions_%s%s.npz" % (tag, suffix))))

            def chk(name, loss, wrt, tight):
                if name not in g:
                    return
                assert abs(float(loss) - float(g[name])) <= 1e-4 * abs(float(g[name])), (tag, suffix, name, float(loss), float(g[name]))
                grads = torch.autograd.grad(loss, list(wrt.values()), allow_unused=True)
                values[tag + suffix + ":" + name] = (loss.detach().cpu(), {k: gr.detach().cpu() for k, gr in zip(wrt, grads) if gr is not None})
                worst = 0.0
                for (k, _), gr in zip(wrt.items(), grads):
                    key = name + ".grad." + k
                    if gr is None:
                        assert key not in g
                        continue
                    ref = torch.from_numpy(g[key])
                    worst = max(worst, rel(gr, ref))
                    assert _grad_ok(gr, ref, tight), (tag, suffix, name, k, rel(gr, ref))
                res[tag + suffix + ":" + name] = worst
                if not tight and "pose" in wrt:
                    res[tag + suffix + ":" + name + ":elements_at_tap_boundaries"] = _flip_pinned(name, a, list(wrt.keys()), grads, g, ac)

            tight_warp = smooth > 0
            a, _ = _pyr(dev, FB, FH, FW, smooth)
            wrt = {("depth%d" % i): d for i, d in enumerate(a["depth"])}
            wrt.update({("mask%d" % i): m for i, m in enumerate(a["mask"])})
            wrt["pose"] = a["pose"]
            chk("photometric_reconstruction_loss",
                LF.photometric_reconstruction_loss(a["tgt"], a["refs"], a["K"], a["Kinv"], a["depth"], a["mask"], a["pose"],
                                                   wssim=0.997, qch=0.5, align_corners=ac), wrt, tight_warp)
            a, _ = _pyr(dev, FB, FH, FW, smooth)
            wrt = {("depth%d" % i): d for i, d in enumerate(a["depth"])}
            wrt["pose"] = a["pose"]
            chk("photometric_reconstruction_loss_nomask",
                LF.photometric_reconstruction_loss(a["tgt"], a["refs"], a["K"], a["Kinv"], a["depth"], [None] * 6, a["pose"],
                                                   wssim=0.5, qch=0.5, lambda_oob=0.3, align_corners=ac), wrt, tight_warp)
            a, _ = _pyr(dev, FB, FH, FW, smooth)
            wrt = {("flow_fwd%d" % i): f for i, f in enumerate(a["ff"])}
            wrt.update({("flow_bwd%d" % i): f for i, f in enumerate(a["fb"])})
            wrt.update({("mask%d" % i): m for i, m in enumerate(a["mask"])})
            # flow warps take no P: coordinates are bit-identical to the reference's -> tight on noise too
            chk("photometric_flow_loss",
                LF.photometric_flow_loss(a["tgt"], a["refs"][1:3], [a["fb"], a["ff"]], [1 - m[:, 1:3] for m in a["mask"]],
                                         wssim=0.997, qch=0.5, align_corners=ac), wrt, True)
            if smooth:
                continue
            mk = {("mask%d" % i): m for i, m in enumerate(a["mask"])}
            chk("explainability_loss", LF.explainability_loss(a["mask"]), mk, True)
            for nm, key in (("depth", "depth"), ("flow_fwd", "ff"), ("mask", "mask")):
                chk("edge_aware_smoothness_loss." + nm, LF.edge_aware_smoothness_loss(a["tgt"], a[key]),
                    {("%s%d" % (nm, i)): t for i, t in enumerate(a[key])}, True)
            with torch.no_grad():
                p = a["pose"].detach()
                cf = [IW.pose2flow(d[:, 0], p[:, 2], a["K"], a["Kinv"]) for d in a["depth"]]
                cb = [IW.pose2flow(d[:, 0], p[:, 1], a["K"], a["Kinv"]) for d in a["depth"]]
                tg = LF.consensus_exp_masks(cf, cb, a["ff"], a["fb"], a["tgt"], a["refs"][2], a["refs"][1], wssim=0.997,
                                            wrig=1.0, align_corners=ac)
                for i, t in enumerate(tg):
                    assert float(np.mean(t.cpu().numpy().astype(np.uint8) != g["consensus_exp_masks.%d" % i])) <= 5e-3
                occ = LF.depth_occlusion_masks(a["depth"][0], p, a["K"], a["Kinv"])
                assert float(np.mean(occ.cpu().numpy().astype(np.uint8) != g["depth_occlusion_masks.0"])) <= 1e-4
                rf = [torch.from_numpy(g["pose2flow_fullK.%d" % i]).to(dev) - y for i, y in enumerate(a["ff"])]
                rf = [x.abs() for x in rf]
                rb = [(x - y).abs() for x, y in zip(cb, a["fb"])]
                tgt_ref = [torch.from_numpy(g["consensus_exp_masks.%d" % i].astype(np.float32)).to(dev) for i in range(6)]
            # THRESH-ed census masks are discontinuous in the rigid flow: compare the loss only loosely on this term's
            # inputs that came through this device's P (rb); exact reference values are used for rf
            l5 = LF.consensus_depth_flow_mask(a["mask"], rb, rf, tgt_ref, tgt_ref, THRESH=0.5, wbce=0.5)
            values[tag + suffix + ":consensus_depth_flow_mask"] = (l5.detach().cpu(), {})
            assert abs(float(l5) - float(g["consensus_depth_flow_mask"])) <= 1e-3 * abs(float(g["consensus_depth_flow_mask"]))
    return res


def check_losses_chunked(dev, golden_dir):
    """Job tables longer than a launch holds: check_losses_vs_golden again with loss_functions.MAX_JOBS = 5 -- 5 divides none of
    the 24, 18 and 12 rows of the step's tables, and the rigid loss runs one level per chunk -- under the same bars against the
    reference's fixtures.  The photometric losses add their terms one by one in job order (k_photo_finalize_jobs), so they equal
    their unchunked values bit for bit; the terms summed by k_reduce_add (one reduction per chunk instead of one over all rows)
    and the pose gradient (one partial gradient per chunk, added in chunk order) are printed against the unchunked values."""
    full, cut = {}, {}
    assert LF.MAX_JOBS == 24
    check_losses_vs_golden(dev, golden_dir, values=full)
    LF.MAX_JOBS = 5
    try:
        res = check_losses_vs_golden(dev, golden_dir, values=cut)
    finally:
        LF.MAX_JOBS = 24
    assert sorted(full) == sorted(cut) and len(full) >= 20
    for case in sorted(full):
        (l0, g0), (l1, g1) = full[case], cut[case]
        if "photometric" in case:
            assert torch.equal(l0, l1), (case, float(l0), float(l1))
        else:
            print("%-50s loss %.9g, chunked %.9g (diff %.2e)" % (case, float(l0), float(l1), abs(float(l0) - float(l1))))
        for k in g0:
            if k == "pose":
                print("%-50s pose gradient: chunked vs whole, rel %.2e" % (case, rel(g1[k], g0[k])))
    return res


def check_losses_rare(dev, golden_dir):
    """Loss calls no training configuration makes, against tests/golden/loss_rare.npz (the unmodified reference, low-pass frames,
    align_corners=False; oracle/make_golden.py rare_level): rotation_mode='quat', masks with more channels than reference frames,
    a mask list of mixed channel counts.  Bars of check_losses_vs_golden: 1e-4 rel on the loss, the tight gradient bar."""
    import os
    from oracle.make_golden import rare_calls, rare_inputs
    g = dict(np.load(os.path.join(golden_dir, "loss_rare.npz")))
    x = rare_inputs()
    x = {k: (to(dev, v) if k not in ("pyr", "pose") else v) for k, v in x.items()}
    res, seen = {}, 0
    for name, loss, wrt in rare_calls(LF, x, lambda t: leaf(t, dev)):
        assert abs(float(loss) - float(g[name])) <= 1e-4 * abs(float(g[name])), (name, float(loss), float(g[name]))
        grads = torch.autograd.grad(loss, list(wrt.values()), allow_unused=True)
        worst = 0.0
        for k, gr in zip(wrt, grads):
            key = name + ".grad." + k
            if gr is None:
                assert key not in g, key
                continue
            ref = torch.from_numpy(g[key])
            assert gr.shape == ref.shape, (key, gr.shape, ref.shape)
            worst = max(worst, rel(gr, ref))
            assert _grad_ok(gr, ref, True), (name, k, rel(gr, ref))
            if name == "photometric_flow_loss_wide_masks" and k.startswith("mask"):
                assert gr.shape[1] == 4 and not bool(gr[:, 2:].ne(0).any()), (name, k)      # channels no term reads: exactly zero
                assert bool(gr[:, :2].ne(0).any()), (name, k)
            seen += 1
        res[name] = (float(loss), worst)
        print("%-40s loss %.8g (reference %.8g), worst gradient rel %.2e" % (name, float(loss), float(g[name]), worst))
    assert len(res) == 3 and seen == sum(1 for k in g if ".grad." in k)
    return res


# ----------------------------------------------------------------------------------------------------------------------
# convolutions (the networks' hot kernels): engine vs torch fp32 on the CPU (the reference's nn.Conv2d / ConvTranspose2d)
CONV_CASES = [  # B, Cin, H, W, Cout, k, stride, pad, act, bias, residual
    (2, 3, 16, 20, 32, 7, 2, 3, "relu", True, False),
    (2, 16, 9, 13, 40, 3, 1, 1, "lrelu", True, False),
    (1, 20, 8, 10, 2, 3, 1, 1, None, True, False),
    (2, 33, 7, 9, 70, 3, 2, 1, "relu", False, False),
    (2, 24, 6, 7, 24, 3, 1, 1, "relu", False, True),
    (1, 130, 5, 6, 150, 1, 1, 0, None, True, False),
    (2, 8, 10, 12, 1, 3, 1, 1, "sigmoid", True, False),
    (2, 5, 12, 9, 16, 5, 2, 2, "relu", True, False),
    (2, 12, 6, 8, 12, 1, 2, 0, None, False, False),
    (2, 10, 11, 70, 20, 3, 1, 1, "relu", True, False),
    (1, 6, 21, 75, 8, 3, 2, 1, "relu", True, False),
    (2, 64, 5, 40, 64, 3, 1, 1, "relu", False, True),
    (1, 40, 6, 32, 96, 3, 1, 1, "lrelu", True, False),
    # few-channel 3x3 layers on larger maps (prediction heads: <= 4 outputs; their data-gradients: <= 4 reduction channels; a
    # 3-channel input layer)
    (1, 20, 32, 72, 4, 3, 1, 1, "sigmoid", True, False),
    (2, 9, 33, 70, 1, 3, 1, 1, "sigmoid", True, False),
    (1, 16, 40, 64, 2, 3, 1, 1, None, True, False),
    (1, 3, 32, 72, 16, 3, 1, 1, "relu", True, False),
    (2, 2, 35, 66, 5, 3, 1, 1, "lrelu", False, False),
    (2, 7, 9, 13, 3, 3, 1, 1, "sigmoid", True, False),          # odd width: one pixel per work-item in conv_heads.hip
    # maps of <= 4 lattice rows: the pixel tile stacks the rows of 2 / 4 / 8 consecutive images (conv.hip CP::ipt) -- every channel
    # tile (16 / 32 / 64 / 128), a batch that does not fill the last tile, stride 2 onto such a map (and its data-gradient's parity
    # classes), rows that are / are not 16-byte aligned, split-K (deep) and fused epilogues
    (4, 40, 2, 7, 70, 3, 1, 1, "relu", True, True),
    (4, 72, 4, 13, 130, 3, 1, 1, "lrelu", True, False),
    (5, 24, 3, 5, 20, 3, 1, 1, None, True, False),
    (8, 16, 1, 4, 10, 3, 1, 1, "sigmoid", True, False),
    (3, 33, 8, 14, 40, 3, 2, 1, "relu", True, False),
    (4, 20, 4, 8, 24, 3, 2, 1, "relu", False, False),
    (4, 64, 2, 8, 64, 3, 1, 1, "relu", True, False),
    (3, 12, 4, 12, 12, 1, 1, 0, None, True, False),
    (4, 260, 2, 7, 48, 3, 1, 1, "relu", True, False),
]
# 3x3 / stride 1 / pad 1 layers on the Winograd F(2x2, 3x3) kernel (wino.hip; forward and data-gradient): odd map sizes (tiles that
# hang over the border), channel counts that are not multiples of 4 / 8 / 64, residual + every activation, tile blocks that span
# images, split-K over channel chunks (deep layer, few tiles)
CONV_CASES_WINO = [      # (the kernel takes maps whose width is a multiple of 4 with >= 16 tile columns, or exactly 8)
    (2, 64, 5, 40, 64, 3, 1, 1, "relu", False, True),
    (1, 40, 6, 32, 96, 3, 1, 1, "lrelu", True, False),
    (2, 33, 7, 36, 70, 3, 1, 1, "relu", True, False),
    (3, 26, 9, 44, 40, 3, 1, 1, None, False, False),
    (2, 129, 8, 32, 65, 3, 1, 1, "sigmoid", True, False),
    (1, 196, 6, 16, 128, 3, 1, 1, "lrelu", True, False),
    (2, 48, 16, 52, 48, 3, 1, 1, "relu", True, True),
    (4, 256, 4, 16, 130, 3, 1, 1, "relu", True, False),
    (1, 24, 5, 104, 40, 3, 1, 1, "lrelu", True, False),
]
# ... at sizes whose launches are large enough to keep the whole reduction in one workgroup (fused bias / residual / activation
# epilogue in the Winograd kernel): GPU only (the reference is torch on the CPU: a few GFLOP each)
# (smooth epilogues only: among millions of outputs a few pre-activations lie within the summation-order noise of zero, and a
# ReLU / LeakyReLU derivative that flips there moves single gradient elements by O(1) -- in ANY two implementations)
CONV_CASES_WINO_LARGE = [
    (4, 32, 64, 208, 128, 3, 1, 1, None, True, False),
    (4, 64, 64, 208, 64, 3, 1, 1, None, False, True),
    (2, 40, 63, 204, 130, 3, 1, 1, "sigmoid", True, False),
    (4, 128, 32, 104, 128, 3, 1, 1, None, True, True),
    (4, 129, 33, 100, 65, 3, 1, 1, "sigmoid", True, False),
]
# few channels x many pixels (wgrad_thin.hip; the pixel threshold is lowered for the small test maps)
# 3x3 / stride-1 layers on maps whose width is NOT a multiple of 4 (8x26, 4x13 in the step): their weight gradients run on the Winograd
# kernel over zero-padded copies of dY and the input (conv.hip k_pad_rows); smooth epilogues (see CONV_CASES_WINO_LARGE)
CONV_CASES_WINO_PADW = [          # product thresholds (>= 96 channels on both sides, >= 64 tiles)
    (4, 96, 8, 26, 128, 3, 1, 1, None, True, False),
    (4, 100, 4, 13, 96, 3, 1, 1, "sigmoid", True, False),
    (3, 128, 5, 10, 97, 3, 1, 1, None, False, False),
]
# ... and their forward / data-gradient arithmetic on the Winograd kernel over a zero-padded copy of the INPUT (conv.hip plan_conv
# ConvPlan::wpad: always split-K, the epilogue kernel writes the real output): product thresholds (>= 256 channels on both sides)
CONV_CASES_WINO_PADIN = [
    (4, 256, 8, 26, 256, 3, 1, 1, None, True, True),
    (2, 256, 9, 30, 260, 3, 1, 1, "sigmoid", True, False),
]
CONV_CASES_WINO_PADIN_SMALL = [   # emulator sizes (thresholds lowered through the tools switches); 13 -> 16 columns (8 tile columns)
    (2, 20, 6, 26, 24, 3, 1, 1, None, True, False),
    (1, 16, 5, 13, 24, 3, 1, 1, "sigmoid", True, True),
    (3, 24, 4, 30, 40, 3, 1, 1, "relu", True, False),
    (2, 9, 3, 26, 33, 3, 1, 1, "lrelu", False, False),
]
CONV_CASES_WINO_PADW_SMALL = [    # emulator sizes (thresholds lowered through the tools switches)
    (2, 20, 4, 10, 24, 3, 1, 1, None, True, False),
    (2, 33, 5, 13, 40, 3, 1, 1, "sigmoid", True, True),
    (1, 16, 3, 7, 24, 3, 1, 1, None, True, False),
]
# prediction heads (<= 4 output channels from <= 64 inputs) on the VALU kernel of conv_heads.hip (k_conv_thinm; the pixel threshold is
# lowered for the small test maps): 1 / 2 / 4 / 8 channel shares per workgroup, a channel count that does not divide by the shares
CONV_CASES_HEADS = [
    (1, 16, 40, 64, 2, 3, 1, 1, None, True, False),
    (2, 8, 10, 12, 1, 3, 1, 1, "sigmoid", True, False),
    (1, 16, 7, 36, 4, 3, 1, 1, "sigmoid", True, False),
    (2, 40, 8, 16, 4, 3, 1, 1, "relu", True, False),
    (2, 64, 6, 8, 3, 3, 1, 1, "lrelu", False, False),
    (1, 5, 9, 20, 1, 3, 1, 1, None, False, False),
    (1, 37, 5, 24, 2, 3, 1, 1, "sigmoid", True, False),
]
CONV_CASES_THIN = [
    (2, 16, 9, 16, 16, 3, 1, 1, "relu", True, False),
    (2, 17, 6, 20, 16, 3, 1, 1, "lrelu", True, False),
    (1, 16, 7, 36, 4, 3, 1, 1, "sigmoid", True, False),
    (2, 3, 12, 24, 16, 3, 2, 1, "relu", True, False),
    (2, 15, 16, 40, 16, 7, 2, 3, "relu", True, False),
    (1, 32, 6, 16, 32, 7, 1, 3, "relu", True, False),
    (2, 17, 5, 12, 16, 1, 1, 0, None, False, False),
    (2, 16, 10, 24, 32, 5, 2, 2, "relu", True, False),
    (2, 16, 5, 8, 1, 3, 1, 1, "sigmoid", True, False),
    (2, 20, 6, 44, 30, 3, 2, 1, None, True, False),
    (2, 16, 32, 128, 16, 3, 1, 1, "relu", True, False),          # 64 unit ranges: the XCD-swizzled assignment
    (2, 24, 10, 24, 40, 1, 2, 0, None, False, False),            # 1x1 stride-2 shortcut convs of the ResNet blocks
]
CONVT_CASES = [  # B, Cin, H, W, Cout, k, stride, pad, output_padding, act
    (2, 16, 5, 7, 24, 3, 2, 1, 1, "relu"),
    (2, 20, 4, 6, 12, 4, 2, 1, 0, "relu"),
    (1, 40, 3, 5, 40, 3, 2, 1, 1, None),
    (2, 48, 6, 8, 16, 4, 2, 1, 0, "relu"),
    (2, 32, 5, 8, 16, 3, 2, 1, 1, None),
    (4, 24, 2, 7, 16, 3, 2, 1, 1, "relu"),       # stacked tiny maps (see CONV_CASES)
    (3, 40, 1, 4, 40, 4, 2, 1, 0, None),
]


def _torch_act(y, act, a, b):
    import torch.nn.functional as F
    if act == "relu":
        return F.relu(y)
    if act == "lrelu":
        return F.leaky_relu(y, b if b != 0 else 0.2)
    if act == "sigmoid":
        return a * torch.sigmoid(y) + b
    return y


def check_convs(dev, cases=CONV_CASES, tcases=CONVT_CASES, tol=2e-5, seed=0, prepack=False):
    """conv2d / conv_transpose2d forward (+ fused bias / residual / activation epilogue) and all gradients, max-abs
    error relative to the largest reference magnitude <= tol (fp32 MFMA accumulation order differs from the CPU's).
    prepack=True runs every case a second time through the trainer's per-step weight images (cc_repack_table) -- the
    path on which the parity classes of stride-2 data-gradients / transposed convs share one launch."""
    import torch.nn.functional as F
    from cc_amd import ops
    g = torch.Generator().manual_seed(seed)
    passes = 2 if prepack else 1
    ops.packs.reset()

    def rn(*s):
        return torch.randn(*s, generator=g)
    for (B, Cin, H, W, Cout, k, st, pad, act, hb, hr) in cases:
        x0, w0 = rn(B, Cin, H, W), rn(Cout, Cin, k, k) * 0.2
        b0 = rn(Cout) if hb else None
        OH, OW = (H + 2 * pad - k) // st + 1, (W + 2 * pad - k) // st + 1
        r0 = rn(B, Cout, OH, OW) if hr else None
        aa, ab = (10.0, 0.01) if act == "sigmoid" else (1.0, 0.0)
        ins_d = [leaf(t, dev) if t is not None else None for t in (x0, w0, b0, r0)]
        ins_c = [leaf(t, "cpu") if t is not None else None for t in (x0, w0, b0, r0)]
        r = F.conv2d(ins_c[0], ins_c[1], ins_c[2], st, pad)
        if hr:
            r = r + ins_c[3]
        r = _torch_act(r, act, aa, ab)
        go = rn(*r.shape)
        g0 = torch.autograd.grad(r, [t for t in ins_c if t is not None], go)
        for ps in range(passes):
            if ps == 1:
                ops.packs.prepack_all()
            y = ops.conv2d(ins_d[0], ins_d[1], ins_d[2], st, pad, act, ins_d[3], aa, ab)
            g1 = torch.autograd.grad(y, [t for t in ins_d if t is not None], go.to(dev))
            errs = [rel(y, r)] + [rel(a, b) for a, b in zip(g1, g0)]
            assert max(errs) < tol, ((B, Cin, H, W, Cout, k, st, pad, act), ps, errs)
            ops.packs.invalidate()
    for (B, Cin, H, W, Cout, k, st, pad, op, act) in tcases:
        x0, w0, b0 = rn(B, Cin, H, W), rn(Cin, Cout, k, k) * 0.2, rn(Cout)
        ins_d = [leaf(t, dev) for t in (x0, w0, b0)]
        ins_c = [leaf(t, "cpu") for t in (x0, w0, b0)]
        r = _torch_act(F.conv_transpose2d(ins_c[0], ins_c[1], ins_c[2], st, pad, op), act, 1.0, 0.0)
        go = rn(*r.shape)
        g0 = torch.autograd.grad(r, ins_c, go)
        for ps in range(passes):
            if ps == 1:
                ops.packs.prepack_all()
            y = ops.conv_transpose2d(ins_d[0], ins_d[1], ins_d[2], st, pad, op, act)
            g1 = torch.autograd.grad(y, ins_d, go.to(dev))
            errs = [rel(y, r)] + [rel(a, b) for a, b in zip(g1, g0)]
            assert max(errs) < tol, ((B, Cin, H, W, Cout, k, st, pad, op, act), ps, errs)
            ops.packs.invalidate()
    ops.packs.reset()


# Winograd launches that hold the WHOLE reduction (fused epilogue, no split-K) with the non-smooth epilogues the step uses: ReLU /
# LeakyReLU (+ residual) in the forward kernel (EPI_LIN) and `(sum) * act'(y1)` in the data-gradient of the consumer (EPI_GRAD: the
# producer's activation backward deferred into it).  (B, Cin, H, W, C1, C2, act, residual)
CONV_CASES_WINO_ACT = [
    (4, 64, 64, 208, 64, 64, "relu", True),        # 64 x 64 blocks (208 of them) + the 32 x 32 instances of the second layer's gradient
    (4, 128, 32, 104, 128, 96, "lrelu", False),    # 32 x 32 blocks, four waves
    (4, 256, 16, 52, 256, 128, "relu", True),      # 32 x 32 blocks, eight waves (the reduction halved inside the workgroup)
    (2, 32, 64, 208, 32, 48, "lrelu", True),       # 32 output channels: one 32-row block
]
CONV_CASES_WINO_ACT_SMALL = [                      # emulator sizes
    (2, 48, 8, 32, 40, 48, "relu", True),
    (1, 64, 6, 32, 64, 32, "lrelu", False),
]


def check_convs_act_pinned(dev, cases=CONV_CASES_WINO_ACT, tol=2e-5):
    """x -> y1 = act(conv1(x) + b1 [+ res]) -> y2 = conv2(y1) + b2, every gradient, with the activation derivative PINNED: among
    millions of pre-activations a few lie within the summation-order noise of zero, and a ReLU / LeakyReLU derivative that falls the
    other way there moves single gradient elements by O(1) in ANY two implementations.  The reference therefore takes its derivative
    mask from the device's own y1 (> 0); the test asserts that the masks differ only where the reference's pre-activation is within
    1e-5 of zero (relative to the largest), counts those elements, and holds every gradient to the tight bar.  Both forms of the
    activation backward are run: as a pass of its own (the layer's output has a non-conv consumer) and deferred into the consumer's
    data-gradient epilogue (defer / pre_act: the form the tape uses inside the networks)."""
    import torch.nn.functional as F
    from cc_amd import ops
    g = torch.Generator().manual_seed(33)

    def rn(*s):
        return torch.randn(*s, generator=g)
    report = []
    for (B, Cin, H, W, C1, C2, act, hr) in cases:
        slope = 0.0 if act == "relu" else 0.2
        x0, w1, b1 = rn(B, Cin, H, W), rn(C1, Cin, 3, 3) * (1.5 / (3 * Cin ** 0.5)), rn(C1) * 0.3
        w2, b2 = rn(C2, C1, 3, 3) * (1.5 / (3 * C1 ** 0.5)), rn(C2) * 0.3
        r0 = rn(B, C1, H, W) if hr else None
        go = rn(B, C2, H, W)
        with torch.no_grad():
            pre = F.conv2d(x0, w1, b1, 1, 1)
            if hr:
                pre = pre + r0
        for deferred in ((False, True) if not hr else (False,)):      # (the deferred form has no residual operand: _Conv2dFn)
            ops.packs.reset()
            td = [leaf(t, dev) if t is not None else None for t in (x0, w1, b1, r0, w2, b2)]
            if deferred:
                y1 = ops.conv2d(td[0], td[1], td[2], 1, 1, act, None, 1.0, slope, defer=True)
                y2 = ops.conv2d(y1, td[4], td[5], 1, 1, None, pre_act=act, pre_slope=slope)
            else:
                y1 = ops.conv2d(td[0], td[1], td[2], 1, 1, act, td[3], 1.0, slope)
                y2 = ops.conv2d(y1, td[4], td[5], 1, 1, None)
            g1 = torch.autograd.grad(y2, [t for t in td if t is not None], go.to(dev))
            mask = (y1.detach().cpu() > 0)
            flips = mask != (pre > 0)
            nflip = int(flips.sum())
            if nflip:
                assert float(pre[flips].abs().max()) <= 1e-5 * float(pre.abs().max()), ("flip away from zero", float(pre[flips].abs().max()))
            assert nflip <= 1e-4 * pre.numel(), (nflip, pre.numel())
            tc = [leaf(t, "cpu") if t is not None else None for t in (x0, w1, b1, r0, w2, b2)]
            p1 = F.conv2d(tc[0], tc[1], tc[2], 1, 1)
            if hr:
                p1 = p1 + tc[3]
            y1c = torch.where(mask, p1, slope * p1)                  # the activation with the device's derivative mask
            y2c = F.conv2d(y1c, tc[4], tc[5], 1, 1)
            g0 = torch.autograd.grad(y2c, [t for t in tc if t is not None], go)
            errs = [rel(y1, y1c), rel(y2, y2c)] + [rel(a, b) for a, b in zip(g1, g0)]
            assert max(errs) < tol, ((B, Cin, H, W, C1, C2, act, hr), deferred, errs)
            report.append(((B, Cin, H, W, C1, C2, act, hr, deferred), nflip, max(errs)))
    ops.packs.reset()
    return report


def check_conv_groups(dev, tol=2e-5, prepack=True, cases=((2, 6, 9, 14, 20, 12, 1), (1, 3, 12, 20, 16, 24, 2), (2, 40, 5, 8, 136, 16, 1), (1, 32, 4, 16, 72, 8, 1))):
    """Grouped convolution chains (cc_conv2d_*_group: the parallel decoder / feature branches of Back2Future as one launch
    per pass) vs per-branch torch convs: conv(stride s, LeakyReLU, deferred activation backward) -> conv(LeakyReLU) -> conv,
    G = 3 branches with their own inputs and parameters, one branch's output left out of the loss (no gradient: it must drop
    out of the backward launches), all input / weight / bias gradients."""
    import torch.nn.functional as F
    from cc_amd import ops
    g = torch.Generator().manual_seed(21)
    G = 3

    def rn(*s):
        return torch.randn(*s, generator=g)
    for (B, Cin, H, W, C1, C2, st) in cases:
        x0 = [rn(B, Cin, H, W) for _ in range(G)]
        w1 = [rn(C1, Cin, 3, 3) * 0.2 for _ in range(G)]
        b1 = [rn(C1) * 0.3 for _ in range(G)]
        w2 = [rn(C2, C1, 3, 3) * 0.1 for _ in range(G)]
        b2 = [rn(C2) * 0.3 for _ in range(G)]
        w3 = [rn(2, C2, 3, 3) * 0.1 for _ in range(G)]
        b3 = [rn(2) for _ in range(G)]
        flat = x0 + w1 + b1 + w2 + b2 + w3 + b3
        td = [leaf(t, dev) for t in flat]
        tc = [leaf(t, "cpu") for t in flat]

        def split(ts):
            return [ts[i * G:(i + 1) * G] for i in range(7)]
        # reference
        xc, w1c, b1c, w2c, b2c, w3c, b3c = split(tc)
        outs_c = []
        for k in range(G):
            y = F.leaky_relu(F.conv2d(xc[k], w1c[k], b1c[k], st, 1), 0.2)
            y = F.leaky_relu(F.conv2d(y, w2c[k], b2c[k], 1, 1), 0.2)
            outs_c.append(F.conv2d(y, w3c[k], b3c[k], 1, 1))
        go = [rn(*o.shape) for o in outs_c]
        used = [0, 2]                                     # branch 1 gets no gradient
        loss_c = sum((outs_c[k] * go[k]).sum() for k in used)
        wrt_c = [t for i, t in enumerate(tc) if (i % G) in used]
        g0 = torch.autograd.grad(loss_c, wrt_c)
        for ps in range(2 if prepack else 1):
            ops.packs.reset()
            if ps == 1:
                ops.packs.prepack_all()                   # opens registration; second prepack below builds the images
            xd, w1d, b1d, w2d, b2d, w3d, b3d = split(td)

            def run():
                y = ops.conv2d_group(xd, w1d, b1d, st, 1, "lrelu", defer=True)
                y = ops.conv2d_group(y, w2d, b2d, 1, 1, "lrelu", pre_act="lrelu", defer=True)
                return ops.conv2d_group(y, w3d, b3d, 1, 1, None, pre_act="lrelu")
            if ps == 1:
                with torch.no_grad():
                    run()                                 # registers the layers
                ops.packs.prepack_all()
            outs_d = run()
            for k in range(G):
                assert rel(outs_d[k], outs_c[k]) < tol, ("group fwd", (B, Cin, H, W, C1, C2, st), ps, k, rel(outs_d[k], outs_c[k]))
            loss_d = sum((outs_d[k] * go[k].to(dev)).sum() for k in used)
            wrt_d = [t for i, t in enumerate(td) if (i % G) in used]
            g1 = torch.autograd.grad(loss_d, wrt_d)
            errs = [rel(a, b) for a, b in zip(g1, g0)]
            assert max(errs) < tol, ("group grads", (B, Cin, H, W, C1, C2, st), ps, errs)
            ops.packs.invalidate()
    ops.packs.reset()


def check_conv_list(dev, tol=2e-5):
    """cc_conv2d_list: four problems of different shapes and kinds in one call -- a residual + ReLU forward (130 channels),
    a plain forward on another map size, a stride-2 data-gradient with the fused (sum + add) * relu'(mul) epilogue and a
    stride-1 data-gradient accumulating in place under LeakyReLU' -- against torch's convolutions."""
    import torch.nn.functional as F
    from cc_amd import ops
    from tools import launchlist as LL
    g = torch.Generator().manual_seed(5)

    def rn(*s):
        return torch.randn(*s, generator=g)
    ops.packs.reset()
    xa, wa, ba, ra = rn(2, 24, 5, 8), rn(130, 24, 3, 3) * 0.2, rn(130), rn(2, 130, 5, 8)
    xb, wb = rn(1, 70, 9, 14), rn(128, 70, 3, 3) * 0.1
    wc, gyc, mulc, addc = rn(136, 40, 3, 3) * 0.1, rn(2, 136, 5, 6), torch.relu(rn(2, 40, 10, 12)), rn(2, 40, 10, 12)
    wd, gyd, muld, gxd0 = rn(72, 33, 3, 3) * 0.1, rn(2, 72, 6, 7), rn(2, 33, 6, 7), rn(2, 33, 6, 7)
    # a 160-channel wide buffer whose channels 20..59 receive problem C's result (batch-strided output)
    wide = torch.zeros(2, 160, 10, 12)
    d = [t.clone().to(dev) for t in (xa, wa, ba, ra, xb, wb, wc, gyc, mulc, addc, wd, gyd, muld, gxd0, wide)]
    xa_, wa_, ba_, ra_, xb_, wb_, wc_, gyc_, mulc_, addc_, wd_, gyd_, muld_, gxd_, wide_ = d
    ya_ = torch.empty(2, 130, 5, 8, device=dev)
    yb_ = torch.empty(1, 128, 9, 14, device=dev)
    gxc_ = wide_[:, 20:60]
    recs = [LL.conv_record(xa_, wa_, ba_, ra_, ya_, 1, 1, 1),
            LL.conv_record(xb_, wb_, None, None, yb_, 1, 1, 0),
            LL.tconv_record(gyc_, wc_, None, gxc_, 2, 1, 40 * 9, 9, 3, 3, act=1, mul=mulc_, add=addc_),
            LL.tconv_record(gyd_, wd_, None, gxd_, 1, 1, 33 * 9, 9, 3, 3, act=2, mul=muld_, add=gxd_)]
    ll = LL.LaunchList(recs, dev)
    ops.packs.prepack_all()
    ll.run()
    ops.packs.invalidate()
    ref = [F.relu(F.conv2d(xa, wa, ba, 1, 1) + ra), F.conv2d(xb, wb, None, 1, 1),
           (F.conv_transpose2d(gyc, wc, None, 2, 1, 1) + addc) * (mulc > 0).float()]
    rd = F.conv_transpose2d(gyd, wd, None, 1, 1) + gxd0
    ref.append(torch.where(muld > 0, rd, 0.2 * rd))
    errs = [rel(a, b) for a, b in zip((ya_, yb_, gxc_, gxd_), ref)]
    assert max(errs) < tol, errs
    assert float(wide_[:, :20].abs().max()) == 0 and float(wide_[:, 60:].abs().max()) == 0      # the slice's neighbours untouched
    ops.packs.reset()


def check_feature_warp_deterministic(dev, cases=((2, 32, 16, 24), (1, 96, 12, 20), (2, 128, 8, 13))):
    """cc_feature_warp_bwd_det (config.deterministic: the feature-gradient scatter as 64-bit fixed-point integer atomics) against
    the float-atomic kernel: same gradient to 1e-6 of its magnitude, accumulation onto an existing gradient, and two runs of
    the deterministic form bit for bit (flows of several pixels, many targets landing on the same source pixel: border
    clamping)."""
    from cc_amd._lib import engine, STREAM
    E = engine()
    g = torch.Generator().manual_seed(17)
    for (B, C, H, W) in cases:
        feat = torch.randn(B, C, H, W, generator=g).to(dev)
        flow = (torch.randn(B, 2, H, W, generator=g) * 6.0).to(dev)          # many samples beyond the border (clamped)
        gout = (torch.randn(B, C, H, W, generator=g) * 1e-4).to(dev)
        base = torch.randn(B, C, H, W, generator=g).to(dev) * 1e-4
        ref = torch.zeros_like(feat)
        gflow0 = torch.empty_like(flow)
        E.call("cc_feature_warp_bwd", gout, feat, flow, gflow0, ref, B, C, H, W, 0, 0.625, STREAM)
        outs = []
        for rep in range(2):
            ws = torch.empty(int(E.call("cc_feature_warp_bwd_det_ws_bytes", B, C, H, W)), dtype=torch.uint8, device=dev)
            got, gflow1 = torch.empty_like(feat), torch.empty_like(flow)
            E.call("cc_feature_warp_bwd_det", gout, feat, flow, gflow1, got, ws, B, C, H, W, 0, 0.625, 0, STREAM)
            outs.append(got)
            assert torch.equal(gflow0, gflow1)
        assert torch.equal(outs[0], outs[1])
        assert rel(outs[0], ref) < 1e-6, ((B, C, H, W), rel(outs[0], ref))
        acc = base.clone()
        ws = torch.empty(int(E.call("cc_feature_warp_bwd_det_ws_bytes", B, C, H, W)), dtype=torch.uint8, device=dev)
        E.call("cc_feature_warp_bwd_det", gout, feat, flow, None, acc, ws, B, C, H, W, 0, 0.625, 1, STREAM)
        assert rel(acc, base + ref) < 1e-6


def check_pixel2cam_cam2pixel_grads(dev, B=2, H=20, W=28):
    """The stand-alone pixel2cam / cam2pixel (inverse_warp.py:31-79) under autograd: outputs and ALL gradients (depth, K^-1,
    camera points, rotation, translation; 'zeros' rewrite and the no-rotation / no-translation switches) of the HIP kernels
    against the oracle's restatement of the reference formulas."""
    g = torch.Generator().manual_seed(4)
    depth = torch.rand(B, H, W, generator=g) * 5 + 0.5
    _, _, K, Kinv = syn.sample(B, H, W, seed=1)
    pose = torch.randn(B, 6, generator=g) * 0.05
    P = G.projection(pose, K)
    for mode, use_rot, use_tr in (("zeros", True, True), ("border", True, True), ("zeros", False, True), ("zeros", True, False)):
        outs = []
        for side in ("dev", "cpu"):
            d_ = depth.clone().to(dev if side == "dev" else "cpu").requires_grad_(True)
            ki = Kinv.clone().to(d_.device).requires_grad_(True)
            rot = P[:, :, :3].clone().contiguous().to(d_.device).requires_grad_(True) if use_rot else None
            tr = P[:, :, 3:].clone().contiguous().to(d_.device).requires_grad_(True) if use_tr else None
            if side == "dev":
                cam = IW.pixel2cam(d_, ki)
                grid = IW.cam2pixel(cam, rot, tr, mode)
            else:
                cam = G.pixel2cam(d_, ki)
                grid = G.cam2pixel(cam, rot, tr, mode)
            wgt = torch.randn(grid.shape, generator=torch.Generator().manual_seed(9)).to(grid.device)
            wrt = [t for t in (d_, ki, rot, tr) if t is not None]
            gs = torch.autograd.grad((grid * wgt).sum() + (cam * cam).sum() * 1e-3, wrt)
            outs.append((cam.detach().cpu(), grid.detach().cpu(), [x.cpu() for x in gs]))
        (c1, g1, gr1), (c0, g0, gr0) = outs
        assert rel(c1, c0) < 1e-6 and frac_bad(g1, g0, 1e-5, 1e-5) < 1e-3
        for a, b in zip(gr1, gr0):
            assert rel(a, b) < 2e-4, (mode, use_rot, use_tr, rel(a, b))


def check_corr(dev, cases=((2, 8, 6, 12), (1, 5, 7, 13), (2, 12, 5, 8), (1, 33, 9, 20))):
    """9x9 cost volume (Back2Future): plain `correlate` and the fused pair with the idx_fwd / idx_bwd channel
    permutations, forward and all gradients, vs the oracle; W % 4 == 0 runs the register-blocked kernels, other widths
    the scalar ones."""
    from cc_amd import ops
    from oracle.corr import correlate9
    idx = [k for n in range(80, 71, -1) for k in range(n, -1, -9)]          # models/back2future.py:56-57
    idx_b = list(reversed(idx))
    g = torch.Generator().manual_seed(3)
    for (B, C, H, W) in cases:
        a0, b0, c0 = (torch.randn(B, C, H, W, generator=g) for _ in range(3))
        ad, bd, cd = leaf(a0, dev), leaf(b0, dev), leaf(c0, dev)
        ac, bc, cc_ = leaf(a0, "cpu"), leaf(b0, "cpu"), leaf(c0, "cpu")
        o = ops.correlate(ad, bd)
        r = correlate9(ac, bc)
        assert rel(o, r) < 2e-6, ("correlate", (B, C, H, W), rel(o, r))
        go = torch.randn(r.shape, generator=g)
        g1 = torch.autograd.grad(o, [ad, bd], go.to(dev))
        g0 = torch.autograd.grad(r, [ac, bc], go)
        assert max(rel(x, y) for x, y in zip(g1, g0)) < 5e-6, ("correlate grads", (B, C, H, W))
        o = ops.correlation_pair(ad, bd, cd, idx, idx_b)
        r = torch.cat((correlate9(ac, bc).index_select(1, torch.tensor(idx)),
                       correlate9(ac, cc_).index_select(1, torch.tensor(idx_b))), 1)
        assert rel(o, r) < 2e-6, ("pair", (B, C, H, W), rel(o, r))
        go = torch.randn(r.shape, generator=g)
        g1 = torch.autograd.grad(o, [ad, bd, cd], go.to(dev))
        g0 = torch.autograd.grad(r, [ac, bc, cc_], go)
        assert max(rel(x, y) for x, y in zip(g1, g0)) < 5e-6, ("pair grads", (B, C, H, W), [rel(x, y) for x, y in zip(g1, g0)])


def check_upsample2x(dev, cases=((2, 1, 5, 8, 1.0), (1, 2, 3, 6, -0.625), (2, 2, 16, 26, 20.0), (1, 1, 1, 2, 1.0), (2, 2, 4, 13, 0.625), (1, 1, 3, 1, 1.0))):
    """scale * F.interpolate(x, scale_factor=2, 'bilinear', align_corners=False) (csrc/resize.hip) and its adjoint vs ATen."""
    import torch.nn.functional as F
    from cc_amd import ops
    g = torch.Generator().manual_seed(9)
    for (B, C, H, W, sc) in cases:
        x0 = torch.randn(B, C, H, W, generator=g)
        xd, xc = leaf(x0, dev), leaf(x0, "cpu")
        y = ops.upsample_bilinear2x(xd, sc)
        r = sc * F.interpolate(xc, scale_factor=2, mode="bilinear", align_corners=False)
        assert rel(y, r) < 1e-6, ("up2x", (B, C, H, W), rel(y, r))
        go = torch.randn(r.shape, generator=g)
        g1 = torch.autograd.grad(y, [xd], go.to(dev))[0]
        g0 = torch.autograd.grad(r, [xc], go)[0]
        assert rel(g1, g0) < 2e-6, ("up2x grad", (B, C, H, W), rel(g1, g0))


def check_batch_norm(dev, cases=((2, 5, 7, 12), (3, 16, 9, 13), (2, 8, 32, 64), (2, 3, 96, 128), (4, 2, 80, 104))):
    """Training-mode BatchNorm2d (csrc/bnorm.hip) vs ATen on the CPU: output, running statistics and all gradients;
    cases on both sides of the 16 k values-per-channel switch between the one-launch and the three-launch kernels."""
    import torch.nn.functional as F
    from cc_amd import ops
    g = torch.Generator().manual_seed(5)
    for (B, C, H, W) in cases:
        x0 = torch.randn(B, C, H, W, generator=g) * 2.0 + 0.7
        w0, b0 = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
        rm0, rv0 = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
        xd, wd, bd = leaf(x0, dev), leaf(w0, dev), leaf(b0, dev)
        xc, wc, bc = leaf(x0, "cpu"), leaf(w0, "cpu"), leaf(b0, "cpu")
        rmd, rvd, rmc, rvc = rm0.clone().to(dev), rv0.clone().to(dev), rm0.clone(), rv0.clone()
        y = ops._BNTrainFn.apply(xd, wd, bd, rmd, rvd, 0.1, 1e-5)
        r = F.batch_norm(xc, rmc, rvc, wc, bc, True, 0.1, 1e-5)
        assert rel(y, r) < 2e-6, ("bn out", (B, C, H, W), rel(y, r))
        assert rel(rmd, rmc) < 2e-6 and rel(rvd, rvc) < 2e-6, ("bn running stats", rel(rmd, rmc), rel(rvd, rvc))
        go = torch.randn(r.shape, generator=g)
        g1 = torch.autograd.grad(y, [xd, wd, bd], go.to(dev))
        g0 = torch.autograd.grad(r, [xc, wc, bc], go)
        errs = [rel(a, b) for a, b in zip(g1, g0)]
        assert max(errs) < 1e-5, ("bn grads", (B, C, H, W), errs)
        # eval mode (running statistics; the validation loops): output and input gradient, statistics untouched
        rm1, rv1 = rmd.clone(), rvd.clone()
        ye = ops.batch_norm(xd, wd.detach(), bd.detach(), rmd, rvd, None, False, 0.1, 1e-5)
        re = F.batch_norm(xc, rmc, rvc, wc.detach(), bc.detach(), False, 0.1, 1e-5)
        assert rel(ye, re) < 2e-6, ("bn eval out", (B, C, H, W), rel(ye, re))
        assert torch.equal(rm1, rmd) and torch.equal(rv1, rvd)
        ge1, = torch.autograd.grad(ye, [xd], go.to(dev))
        ge0, = torch.autograd.grad(re, [xc], go)
        assert rel(ge1, ge0) < 2e-6, ("bn eval grad", (B, C, H, W), rel(ge1, ge0))
        # ... and with affine parameters that still train in eval mode (nn.BatchNorm2d allows it): all three gradients
        ye2 = ops.batch_norm(xd, wd, bd, rmd, rvd, None, False, 0.1, 1e-5)
        re2 = F.batch_norm(xc, rmc, rvc, wc, bc, False, 0.1, 1e-5)
        ga1 = torch.autograd.grad(ye2, [xd, wd, bd], go.to(dev))
        ga0 = torch.autograd.grad(re2, [xc, wc, bc], go)
        errs = [rel(a, b) for a, b in zip(ga1, ga0)]
        assert max(errs) < 1e-5, ("bn eval affine grads", (B, C, H, W), errs)
    with pytest.raises(ValueError):          # torch's own check: one value per channel cannot be normalised
        ops.batch_norm(torch.zeros(1, 3, 1, 1, device=dev), None, None, None, None, None, True, 0.1, 1e-5)


def check_corr_patch(dev, cases=((2, 6, 9, 14, 5, 1), (1, 4, 12, 10, 7, 2), (1, 3, 6, 7, 21, 2))):
    """General P x P / dilation-D cost volume (FlowNetC6) vs the oracle's restatement of spatial_correlation_sample."""
    from cc_amd import ops
    from oracle.corr import correlation_volume
    g = torch.Generator().manual_seed(11)
    for (B, C, H, W, P, D) in cases:
        a0, b0 = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
        ad, bd, ac, bc = leaf(a0, dev), leaf(b0, dev), leaf(a0, "cpu"), leaf(b0, "cpu")
        o = ops.correlate_patch(ad, bd, P, D)
        r = correlation_volume(ac, bc, P, D).reshape(B, P * P, H, W) / C
        assert rel(o, r) < 2e-6, ("corr patch", (B, C, H, W, P, D), rel(o, r))
        go = torch.randn(r.shape, generator=g)
        g1 = torch.autograd.grad(o, [ad, bd], go.to(dev))
        g0 = torch.autograd.grad(r, [ac, bc], go)
        assert max(rel(x, y) for x, y in zip(g1, g0)) < 5e-6, ("corr patch grads", (B, C, H, W, P, D))


def check_sum_strided(dev, cases=None):
    """cc_sum_strided: out (=, +=) sum of n <= 8 [B, C, H, W] tensors that are channel slices of wider buffers (own batch strides),
    16-byte and scalar paths -- against the same sum in torch, bit for bit (same left-to-right order)."""
    import ctypes
    from cc_amd import ops
    E = ops.engine()
    g = torch.Generator().manual_seed(13)
    cases = cases or ((2, 4, 6, 8, 2, 0), (2, 3, 5, 7, 3, 1), (1, 2, 8, 12, 8, 0), (3, 2, 4, 4, 5, 1), (2, 6, 9, 16, 1, 1))
    worst = 0.0
    for (B, C, H, W, n, accumulate) in cases:
        parts, keep = [], []
        for k in range(n):
            extra = (k % 3)
            full = torch.randn(B, C + extra, H, W, generator=g).to(dev)
            keep.append(full)
            parts.append(full[:, extra:] if k % 2 == 0 else full[:, :C])
        wide = torch.randn(B, C + 2, H, W, generator=g).to(dev)
        out = wide[:, 1:1 + C]
        want = out.clone() if accumulate else None
        acc = parts[0].clone()
        for p in parts[1:]:
            acc = acc + p
        want = (want + acc) if accumulate else acc
        src = (ctypes.c_long * n)(*[p.data_ptr() for p in parts])
        sbs = (ctypes.c_long * n)(*[p.stride(0) for p in parts])
        guard = wide.clone()
        E.call("cc_sum_strided", n, ctypes.addressof(src), ctypes.addressof(sbs), out, out.stride(0), B, C * H * W, accumulate, ops.STREAM)
        assert torch.equal(out.cpu(), want.cpu()), (B, C, H, W, n, accumulate, float((out - want).abs().max()))
        assert torch.equal(wide[:, 0].cpu(), guard[:, 0].cpu()) and torch.equal(wide[:, 1 + C:].cpu(), guard[:, 1 + C:].cpu())
        worst = max(worst, float((out - want).abs().max()))
    return {"sum_strided": worst}


def check_bias_grad_table(dev, cases=None, tol=2e-5):
    """cc_bias_grad_defer + cc_bias_grad_table (+ the parked second stage, cc_wgrad_reduce_table kind 4): the bias gradients of
    many layers in one launch = the (n, h, w) sums of the pre-activation gradients accumulated onto the existing bias gradients --
    small maps (written directly), chunked planes, planes that are not a multiple of four, channel slices of a larger buffer
    (batch-strided), and more than 32 jobs (two launches)."""
    import ctypes
    from cc_amd import ops
    E = ops.engine()
    g = torch.Generator().manual_seed(11)
    cases = cases or ((2, 16, 9, 13, 0), (2, 8, 64, 160, 0), (1, 130, 5, 6, 0), (2, 4, 33, 70, 3), (3, 24, 12, 40, 8), (2, 1, 128, 130, 0),
                      (4, 3, 8, 8, 0))
    cases = tuple(cases) * 6 if len(cases) * 6 > 32 else tuple(cases)
    jobs, reds, keep, want, gbs = [], [], [], [], []
    for (B, C, H, W, extra) in cases:
        full = torch.randn(B, C + extra, H, W, generator=g).to(dev)
        gy = full[:, extra:]                                   # a channel slice: batch stride (C + extra) * H * W
        gb = torch.randn(C, generator=g).to(dev)
        want.append(gb.double().cpu() + gy.double().sum((0, 2, 3)).cpu())
        ws = torch.empty(max(E.call("cc_act_bwd_ws_bytes", C) // 4, 4), device=dev, dtype=torch.float32)
        job, red, nred = (ctypes.c_long * 12)(), (ctypes.c_long * 16)(), ctypes.c_int(0)
        E.call("cc_bias_grad_defer", gy, gb, ws, B, C, H, W, (C + extra) * H * W, 1, ctypes.addressof(job), ctypes.addressof(red),
               ctypes.addressof(nred))
        jobs.extend(job[:])
        if nred.value:
            reds.extend(red[:])
        keep.append((full, ws))
        gbs.append(gb)
    assert len(jobs) // 12 > 32 and reds, "the cases must cover two table launches and the chunked second stage"
    arr = (ctypes.c_long * len(jobs))(*jobs)
    E.call("cc_bias_grad_table", ctypes.addressof(arr), len(jobs) // 12, ops.STREAM)
    arr2 = (ctypes.c_long * len(reds))(*reds)
    E.call("cc_wgrad_reduce_table", ctypes.addressof(arr2), len(reds) // 16, ops.STREAM)
    worst = 0.0
    for gb, w in zip(gbs, want):
        err = float((gb.double().cpu() - w).abs().max() / (w.abs().max() + 1e-30))
        worst = max(worst, err)
        assert err <= tol, err
    return {"bias_grad_table": worst}


def check_concat_gradient_slices(dev, tol=2e-5):
    """The producers of a torch.cat receive narrow() views of the concat gradient: conv / transposed conv (with activation) and
    the x2 up-sampling read them in place through the kernels' batch-stride arguments (ops._slice_or_c) -- same gradients as
    stock torch, and no contiguous copy of the slice is made."""
    import torch.nn.functional as F
    from cc_amd import ops
    g = torch.Generator().manual_seed(5)
    B, H, W = 2, 8, 12
    x1 = torch.randn(B, 8, H, W, generator=g).to(dev).requires_grad_(True)
    x2 = torch.randn(B, 12, H // 2, W // 2, generator=g).to(dev).requires_grad_(True)
    x3 = torch.randn(B, 4, H // 2, W // 2, generator=g).to(dev).requires_grad_(True)
    w1 = (torch.randn(8, 8, 3, 3, generator=g) * 0.2).to(dev).requires_grad_(True)
    b1 = torch.randn(8, generator=g).to(dev).requires_grad_(True)
    w2 = (torch.randn(12, 8, 3, 3, generator=g) * 0.2).to(dev).requires_grad_(True)
    wo = (torch.randn(5, 20, 3, 3, generator=g) * 0.2).to(dev).requires_grad_(True)
    seen = []
    orig = ops._slice_or_c

    def spy(t):
        r = orig(t)
        seen.append(not r[0].is_contiguous())
        return r
    ops._slice_or_c = spy
    try:
        a = ops.conv2d(x1, w1, b1, 1, 1, act="relu")
        b = ops.conv_transpose2d(x2, w2, None, 2, 1, 1, act="relu")
        c = ops.upsample_bilinear2x(x3, 2.0)
        y = ops.conv2d(torch.cat((a, b, c), 1), wo, None, 1, 1)
        (y * y).sum().backward()
    finally:
        ops._slice_or_c = orig
    got = [t.grad.clone() for t in (x1, x2, x3, w1, b1, w2, wo)]
    for t in (x1, x2, x3, w1, b1, w2, wo):
        t.grad = None
    a = F.relu(F.conv2d(x1, w1, b1, 1, 1))
    b = F.relu(F.conv_transpose2d(x2, w2, None, 2, 1, 1))
    c = 2.0 * F.interpolate(x3, scale_factor=2, mode="bilinear", align_corners=False)
    y = F.conv2d(torch.cat((a, b, c), 1), wo, None, 1, 1)
    (y * y).sum().backward()
    for n, u, t in zip(("x1", "x2", "x3", "w1", "b1", "w2", "wo"), got, (x1, x2, x3, w1, b1, w2, wo)):
        err = float((u - t.grad).abs().max() / (t.grad.abs().max() + 1e-30))
        assert err < tol, (n, err)
    assert len(seen) == 3
    if torch.device(dev).type == "cuda":
        assert all(seen), seen          # every producer read its slice in place (CPU slices may miss the 16-byte alignment)


def check_adam(dev, n=10007, steps=3):
    """cc_adam_step against torch.optim.Adam (betas (0.9, 0.999), eps 1e-8, no weight decay: train.py:307-310) over several steps
    with a gradient scale, and cc_adam_step_segment: the update of [0, cut) with the tick followed by [cut, n) without it is bit
    for bit the one-launch update (the data-parallel step updates the big gradient segment while the small one is still being
    exchanged)."""
    from cc_amd._lib import engine, STREAM
    E = engine()
    g = torch.Generator().manual_seed(9)
    p0 = torch.randn(n, generator=g)
    ref_p = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([ref_p], lr=2e-4, betas=(0.9, 0.999), eps=1e-8)
    mk = lambda: [t.to(dev) for t in (p0.clone(), torch.zeros(n), torch.zeros(n), torch.zeros(1))]
    pa, ma, va, sa = mk()       # one launch
    pb, mb, vb, sb = mk()       # two segments
    pc, mc, vc, sc = mk()       # round 6: cc_adam_tick first, then three segments without a tick, last one first (per-network pipeline)
    cut = (n // 3) // 4 * 4
    scale = 0.5
    for _ in range(steps):
        grad = torch.randn(n, generator=g)
        ref_p.grad = (grad * scale).clone()
        opt.step()
        gd = grad.to(dev)
        E.call("cc_adam_step", pa, gd, ma, va, sa, n, 2e-4, 0.9, 0.999, 1e-8, scale, STREAM)
        E.call("cc_adam_step_segment", pb[:cut], gd[:cut], mb[:cut], vb[:cut], sb, cut, 2e-4, 0.9, 0.999, 1e-8, scale, 1, STREAM)
        E.call("cc_adam_step_segment", pb[cut:], gd[cut:], mb[cut:], vb[cut:], sb, n - cut, 2e-4, 0.9, 0.999, 1e-8, scale, 0, STREAM)
        E.call("cc_adam_tick", sc, STREAM)
        cut2 = cut + (n - cut) // 2 // 4 * 4
        for lo, hi in ((cut2, n), (0, cut), (cut, cut2)):
            E.call("cc_adam_step_segment", pc[lo:hi], gd[lo:hi], mc[lo:hi], vc[lo:hi], sc, hi - lo, 2e-4, 0.9, 0.999, 1e-8, scale, 0, STREAM)
    assert float(sa) == steps and float(sb) == steps and float(sc) == steps
    assert torch.equal(pa.cpu(), pb.cpu()) and torch.equal(ma.cpu(), mb.cpu()) and torch.equal(va.cpu(), vb.cpu())
    assert torch.equal(pa.cpu(), pc.cpu()) and torch.equal(ma.cpu(), mc.cpu()) and torch.equal(va.cpu(), vc.cpu())
    err = float((pa.cpu() - ref_p.detach()).abs().max())
    assert err <= 1e-6, err          # a few ulp (different but equivalent operation order: lr / bc1 folded into the step size)


WGRAD_LIST_SHAPES = [(2, 12, 9, 14, 20, 3, 2, 1), (2, 24, 6, 10, 150, 1, 1, 0), (1, 40, 5, 7, 33, 3, 1, 1), (2, 8, 12, 16, 16, 5, 2, 2),
                     (2, 130, 2, 3, 140, 3, 1, 1), (2, 16, 8, 8, 24, 4, 2, 1), (2, 48, 6, 16, 64, 3, 1, 1)]
# 3x3 / stride-1 layers that take the Winograd weight-gradient kernel (thresholds lowered by the caller): their launches are parked
# too and share multi-geometry launches (wino_wgrad.hip k_wino_wgrad_multi) -- different channel counts / map sizes / split counts,
# a G = 2 group (index 1), a width that is not a multiple of 4 (zero-padded copies first), next to a generic-kernel problem
WGRAD_LIST_SHAPES_WINO = [(2, 48, 6, 16, 64, 3, 1, 1), (1, 20, 8, 24, 40, 3, 1, 1), (2, 33, 5, 13, 40, 3, 1, 1), (2, 16, 4, 8, 24, 3, 1, 1),
                          (2, 12, 9, 14, 20, 3, 2, 1), (1, 70, 9, 32, 130, 3, 1, 1)]


# thin layers (<= 32 channels a side, >= 8192 output pixels, width a multiple of 4: wgrad_thin.hip) inside a list: problems of one kernel
# instance share launches (k_wgrad_thin_multi) -- three 3x3 / stride-1 problems of different channel counts plus a G = 3 group, two
# 3x3 / stride-2, two 1x1, a 7x7 / stride-2 on its own (the plain kernel), next to a generic-kernel problem
WGRAD_LIST_SHAPES_THIN = [(2, 16, 64, 128, 16, 3, 1, 1), (2, 32, 64, 128, 16, 3, 1, 1), (2, 12, 9, 14, 20, 3, 2, 1), (2, 16, 64, 128, 8, 3, 1, 1),
                          (2, 16, 128, 128, 32, 3, 2, 1), (2, 8, 128, 128, 16, 3, 2, 1), (2, 32, 64, 128, 16, 1, 1, 0), (2, 16, 64, 128, 24, 1, 1, 0),
                          (2, 8, 128, 128, 16, 7, 2, 3), (1, 17, 128, 128, 16, 3, 1, 1)]


def check_wgrad_list(dev, tol=2e-5, shapes=None, groups=None):
    """cc_conv2d_wgrad_list (ops._wgrad_list: what a backward stage's weight-gradient queue flushes at its end): groups of different
    shapes in one call -- stride-2 / 1x1 / small-map layers on the generic kernel (k_wgrad_multi: several per launch), direct-mode
    problems (no split) next to split ones, a G = 2 group, a weight that occurs twice (its two accumulations must not share a
    launch), and 3x3 / stride-1 layers that take other kernels inside the same list -- against torch's convolution weight
    gradients, accumulated into pre-filled buffers."""
    import torch.nn.functional as F
    from cc_amd import ops
    g = torch.Generator().manual_seed(33)

    def rn(*s):
        return torch.randn(*s, generator=g)

    def ref_grad(x, gy, shape, k, st, pad):
        w = torch.zeros(*shape, requires_grad=True)
        F.conv2d(x, w, None, st, pad).backward(gy)
        return w.grad
    # (B, Cin, H, W, Cout, k, stride, pad)
    shapes = list(shapes or WGRAD_LIST_SHAPES)
    items, want, bufs = [], [], []
    for si_, (B, Cin, H, W, Cout, k, st, pad) in enumerate(shapes):
        G = (groups or {1: 2}).get(si_, 1)          # problems per group (same-shaped layers of one launch): default a G = 2 group at index 1
        OH, OW = (H + 2 * pad - k) // st + 1, (W + 2 * pad - k) // st + 1
        a_l, x_l, gw_l = [], [], []
        for _ in range(G):
            x, gy, init = rn(B, Cin, H, W), rn(B, Cout, OH, OW), rn(Cout, Cin, k, k) * 0.1
            want.append(init + ref_grad(x, gy, (Cout, Cin, k, k), k, st, pad))
            bufs.append(init.clone().to(dev))
            a_l.append(gy.to(dev).contiguous())
            x_l.append(x.to(dev).contiguous())
            gw_l.append(bufs[-1])
        items.append((a_l, x_l, gw_l, (B, Cout, OH, OW, Cout * OH * OW, Cin, H, W, Cin * H * W, k, k, st, pad, Cin * k * k, k * k)))
    # problem 0 once more, with other operands, INTO THE SAME buffer (a weight used twice in one stage)
    B, Cin, H, W, Cout, k, st, pad = shapes[0]
    x2, gy2 = rn(B, Cin, H, W), rn(*items[0][0][0].shape)
    want[0] = want[0] + ref_grad(x2, gy2, (Cout, Cin, k, k), k, st, pad)
    items.append(([gy2.to(dev).contiguous()], [x2.to(dev).contiguous()], [bufs[0]], items[0][3]))
    with StepScope() as scope:
        scope.park_weight_gradients()
        ops._wgrad_list(items)
        ops.wgrad_reduces.flush()
    if dev != "cpu":
        torch.cuda.synchronize()
    for i, (b, w_) in enumerate(zip(bufs, want)):
        err = float((b.cpu() - w_).abs().max()) / max(float(w_.abs().max()), 1e-30)
        assert err <= tol, ("wgrad_list problem %d" % i, err)


# "The query names what runs": (B, Cin, H, W, Cout, k, stride) of a Conv2d layer with pad = k // 2; every geometry is run as the
# forward call, as its data-gradient without and with a prepacked weight image.  The smallest shapes at which each rule of the
# launch-form decision (conv.hip classes_form / dgrad_merged / launch_gg) can go wrong.
KERNEL_NAME_GEOMS = [
    (1, 16, 8, 26, 64, 1, 2), (2, 48, 16, 32, 16, 1, 2), (2, 96, 2, 7, 136, 1, 2),          # 1x1 stride 2: three parity classes are empty
    (1, 16, 8, 26, 64, 3, 2), (2, 48, 16, 32, 136, 3, 2), (2, 3, 16, 32, 16, 3, 2),         # 3x3 stride 2: classes of 4 / 2 / 2 / 1 taps,
    (1, 96, 2, 7, 64, 3, 2),                                                                 # idle tap slots
    (1, 16, 8, 26, 16, 4, 2), (2, 48, 16, 32, 64, 4, 2),                                     # 4x4 stride 2: four classes of 2 x 2 taps
    (1, 3, 16, 32, 16, 7, 2), (2, 16, 8, 26, 64, 7, 2),                                      # 7x7 stride 2: 16 / 12 / 12 / 9 taps
    (2, 16, 2, 7, 64, 3, 2), (2, 48, 2, 7, 16, 3, 1), (2, 16, 2, 7, 16, 4, 2),               # B = 2 on 2x7: stacked tiny maps
    (1, 3, 2, 7, 136, 3, 2), (2, 3, 2, 7, 136, 3, 1), (1, 96, 2, 7, 136, 3, 2),              # 136 -> 3 on 2x7: split-K
    (1, 16, 16, 32, 64, 3, 1), (2, 48, 16, 32, 136, 3, 1), (2, 96, 16, 32, 16, 3, 1),        # 3x3 stride 1 on 16x32: Winograd
    (1, 3, 16, 32, 16, 3, 1), (2, 16, 16, 32, 2, 3, 1), (2, 48, 8, 26, 2, 3, 1),             # <= 4 channels on one side: head kernels
    (1, 3, 8, 26, 64, 3, 1),
]
KERNEL_NAME_GEOMS_PADDED_WINO = [(2, 48, 8, 26, 64, 3, 1), (1, 96, 8, 26, 136, 3, 1)]         # width 26: Winograd over a padded copy
KERNEL_NAME_CALLS = [("fwd", 0), ("fwd", 1), ("dgrad", 0), ("dgrad", 1)]                      # (call, prepacked)
# one per rule, for the GPU run: (geometry, call, prepacked)
KERNEL_NAME_CASES_GPU = [
    ((1, 16, 8, 26, 64, 1, 2), "dgrad", 1), ((2, 48, 16, 32, 136, 3, 2), "dgrad", 1), ((2, 48, 16, 32, 64, 4, 2), "dgrad", 1),
    ((2, 16, 8, 26, 64, 7, 2), "dgrad", 0), ((2, 16, 2, 7, 64, 3, 2), "dgrad", 1), ((1, 3, 2, 7, 136, 3, 2), "dgrad", 1),
    ((2, 48, 16, 32, 136, 3, 1), "fwd", 1), ((2, 16, 16, 32, 2, 3, 1), "fwd", 0),
]


def check_kernel_names(dev, cases):
    """One engine call per case with the timing registry on (tools build): the set of kernel names its scopes record against the
    answer of cc_conv2d_{fwd,dgrad}_kernel.  The recorded set equals {answer without "+splitk"}; a stride > 1 data-gradient without
    a prepacked image runs one launch per parity class, and the answer (class (0, 0)'s kernel) is one of the set.  "+splitk" is in the
    answer exactly when the kernel's name says it writes partial slabs (the last template argument of the single-problem kernels;
    the multi-problem kernels decide per class, their names do not say).  -> [(case, answer, recorded)]"""
    import ctypes
    import re
    from cc_amd import ops
    from cc_amd._lib import engine
    E = engine()
    assert E.fn["cc_is_tools_build"]() == 1
    gen = torch.Generator().manual_seed(0)
    nbuf, tbuf = ctypes.create_string_buffer(128), ctypes.create_string_buffer(1 << 14)
    out = []
    ops.packs.reset()
    for (B, Cin, H, W, Cout, k, st), call, prepacked in cases:
        pad = k // 2
        OH, OW = (H + 2 * pad - k) // st + 1, (W + 2 * pad - k) // st + 1
        x = torch.randn(B, Cin, H, W, generator=gen).to(dev)
        gy = torch.randn(B, Cout, OH, OW, generator=gen).to(dev)
        w = (torch.randn(Cout, Cin, k, k, generator=gen) * 0.2).to(dev)
        if call == "fwd":
            geom = (B, Cin, H, W, Cout, k, k, st, pad, OH, OW)
            src, dst = x, torch.empty_like(gy)
        else:
            geom = (B, Cout, OH, OW, Cin, k, k, st, pad, H, W)
            src, dst = gy, torch.empty_like(x)
        ws = torch.empty(E.call("cc_conv2d_%s_ws_bytes" % call, *geom) // 4 + 64, device=dev, dtype=torch.float32)
        pk = None
        if prepacked:
            pk = ops.packs.ensure(call, w, geom if call == "fwd" else geom + (Cin * k * k, k * k))
            ops.packs.prepack_all()
        E.call("cc_timing_enable", 1)
        if call == "fwd":
            E.call("cc_conv2d_fwd", src, w, None, None, dst, ws, pk, B, Cin, H, W, Cin * H * W, Cout, k, k, st, pad, OH, OW,
                   Cout * OH * OW, Cout * OH * OW, 0, 1.0, 0.0, ops.STREAM)
        else:
            E.call("cc_conv2d_dgrad", src, w, None, dst, ws, pk, B, Cout, OH, OW, Cout * OH * OW, Cin, k, k, st, pad, H, W,
                   Cin * H * W, Cin * k * k, k * k, 0, 1.0, 0.0, ops.STREAM)
        n = E.fn["cc_timing_collect"](ctypes.addressof(tbuf), 1 << 14)
        recorded = {ln.split("\t")[0] for ln in tbuf.raw[:n].decode().splitlines()}
        assert E.fn["cc_conv2d_%s_kernel" % call](*geom, *((1 if pk is not None else 0,) if call == "dgrad" else ()),
                                                  ctypes.addressof(nbuf), 128) == 0
        answer = nbuf.value.decode()
        case = ((B, Cin, H, W, Cout, k, st), call, prepacked, pk is not None)
        print(case, answer, sorted(recorded))
        base = answer[:-len("+splitk")] if answer.endswith("+splitk") else answer
        if call == "dgrad" and st > 1 and pk is None:
            assert base in recorded, (case, answer, recorded)
        else:
            assert recorded == {base}, (case, answer, recorded)
        if re.match(r"k_conv_patch<|k_conv_patch_stk<|k_wino_f2x3", base):
            assert (re.search(r"(\d+)>$", base).group(1) == "1") == answer.endswith("+splitk"), (case, answer)
        out.append((case, answer, recorded))
    ops.packs.reset()
    return out


# ------------------------------------------------------------------ rigid geometry against float64, away from the identity pose
# Every term is computed three times: by the device, by the oracle in fp32 on the host and by the oracle in float64.
#   e_dev = max|dev - f64| / max|f64|,   e_32 = the same for the fp32 oracle,   bar: e_dev <= 4 * e_32 + 2^-23
# Both fp32 sides evaluate the same formulas and differ in summation order, fma contraction and sinf / cosf only: hence the
# margin of 4; 2^-23 is one rounding of the largest element, for the terms where the host's fp32 result happens to be exact.
# Where sampling DECISIONS enter (the 'zeros' rewrite at |xn| = 1, the border clip, the bilinear tap boundaries) the pixels
# within RIGID_DELTA px of one in float64 are left out on all sides (their upstream gradient is zero), at most 2 % of a map.
RIGID_MARGIN = 4.0
RIGID_FLOOR = 2.0 ** -23
RIGID_DELTA = 1e-3
RIGID_MAX_EXCLUDED = 0.02


def _e64(x, ref, keep=None):
    x, ref = x.detach().cpu().double(), ref.detach().cpu().double()
    assert x.shape == ref.shape, (x.shape, ref.shape)
    if keep is not None:
        x, ref = x[keep], ref[keep]
    return float((x - ref).abs().max() / ref.abs().max())


def _leaf_as(t, dt, d="cpu"):
    """a fresh leaf of t's values in dtype dt on device d (never t itself: .to() of the same dtype returns its argument)"""
    return t.detach().to(dt).to(d).clone().requires_grad_(True)


class _RigidTerms:
    """The comparisons of one check: every figure is printed and noted first, the bars are asserted together at the end."""

    def __init__(self, check, prefix="rigid"):
        self.check, self.prefix, self.bad = check, prefix, []

    def term(self, name, v_dev, v_32, v_64, keep=None, floor=RIGID_FLOOR):
        z = v_64.detach() if keep is None else v_64.detach()[keep]
        if float(z.abs().max()) == 0:
            # nothing reaches this term (every coordinate rewritten or clipped): exactly zero on every side, no ratio to take
            for v in (v_dev, v_32):
                v = v.detach().cpu()
                assert float((v if keep is None else v[keep]).abs().max()) == 0, (self.check, name, "not exactly zero")
            print("%-64s exactly zero on all sides" % (self.check + ":" + name))
            return
        e_dev, e_32 = _e64(v_dev, v_64, keep), _e64(v_32, v_64, keep)
        ratio = e_dev / e_32 if e_32 > 0 else float("inf") if e_dev > 0 else 0.0
        key = "%s:%s:%s" % (self.prefix, self.check, name.split(" ")[0])
        _note(key + ":e_dev", e_dev)
        _note(key + ":e_32", e_32)
        ok = e_dev <= RIGID_MARGIN * e_32 + floor
        print("%-64s e_dev %.3e  e_32 %.3e  ratio %6.2f  %s" % (self.check + ":" + name, e_dev, e_32, ratio, "ok" if ok else "OVER THE BAR"))
        if not ok:
            self.bad.append((name, e_dev, e_32))

    def done(self):
        assert not self.bad, (self.check, "e_dev > 4 * e_32 + floor (2^-23; k * 2^-24 for the sums of the ssim checks)", self.bad)


def _rigid_poses(B, R, seed):
    """[B,R,6] (tx,ty,tz,rx,ry,rz): angles U(-pi, pi) per axis, translations N(0, 1); the first rows are the zero pose and the
    angle triples (pi/2,0,0), (0,pi/2,0) (cos(ry) ~ 0), (0,0,pi), (-3,1.5,2.5)."""
    g = torch.Generator().manual_seed(seed)
    n = B * R
    pose = torch.cat((torch.randn(n, 3, generator=g), (torch.rand(n, 3, generator=g) * 2 - 1) * np.pi), 1)
    fixed = torch.tensor([[0, 0, 0], [np.pi / 2, 0, 0], [0, np.pi / 2, 0], [0, 0, np.pi], [-3, 1.5, 2.5]], dtype=torch.float32)
    pose[:5, 3:] = fixed
    pose[0, :3] = 0
    return pose.float().view(B, R, 6).contiguous()


def _rigid_K(B, H=24, W=40):
    """syn.sample's intrinsics, focal lengths and principal point scaled per batch item so that a kernel that reads the K of
    another batch item shows."""
    K = syn.sample(B, H, W, seed=1)[2].clone()
    for b in range(B):
        K[b, :2] *= 1.0 + 0.125 * b
    return K.contiguous()


def _proj(pose, K, kdiv, dt):
    """oracle: pose [N,6], K [N,3,3] -> P [N,12] with rows 0, 1 of K divided by kdiv (loss_functions.py:91), in dtype dt"""
    K = K.to(dt)
    return G.projection(pose.to(dt), torch.cat((K[:, 0:2] / kdiv, K[:, 2:]), dim=1)).reshape(-1, 12)


def _proj_grad(pose, K, kdiv, gP, dt):
    p = pose.detach().to(dt).requires_grad_(True)
    return torch.autograd.grad((_proj(p, K, kdiv, dt) * gP.to(dt)).sum(), p)[0]


def check_rigid_pose_proj(dev):
    """cc_pose_proj_fwd, cc_pose_proj_levels and cc_pose_proj_bwd through the C ABI at arbitrary rotations against float64
    (smooth functions of the pose: nothing is left out)."""
    import ctypes
    from cc_amd._lib import engine, STREAM
    E = engine()
    T = _RigidTerms("proj")
    B, R, L = 3, 4, 3
    N = B * R
    pose, K = _rigid_poses(B, R, seed=11), _rigid_K(B)
    pose_d, K_d = pose.to(dev), K.reshape(B, 9).to(dev)
    pose_flat, K_flat = pose.view(N, 6), K.repeat_interleave(R, 0)                      # sample n = b * R + r
    K_flat_d = K_flat.reshape(N, 9).contiguous().to(dev)
    fwd = {}
    for kdiv in (1.0, 4.0, 32.0):
        P = torch.full((N, 12), float("nan"), device=dev)
        E.call("cc_pose_proj_fwd", pose_d.view(N, 6), 6, K_flat_d, P, N, kdiv, STREAM)
        T.term("fwd kdiv=%g stride=6" % kdiv, P, _proj(pose_flat, K_flat, kdiv, torch.float32), _proj(pose_flat, K_flat, kdiv, torch.float64))
        fwd[kdiv] = P.cpu()
        # a pose[:, r] slice read in place: rows 6R floats apart
        Ps = torch.full((B, R, 12), float("nan"), device=dev)
        for r in range(R):
            Pr = torch.empty(B, 12, device=dev)
            E.call("cc_pose_proj_fwd", pose_d.data_ptr() + 4 * 6 * r, 6 * R, K_d, Pr, B, kdiv, STREAM)
            Ps[:, r] = Pr
        T.term("fwd kdiv=%g stride=6R" % kdiv, Ps.view(N, 12), _proj(pose_flat, K_flat, kdiv, torch.float32),
               _proj(pose_flat, K_flat, kdiv, torch.float64))
        assert torch.equal(Ps.view(N, 12).cpu(), fwd[kdiv]), "the strided read computes something else than the dense one"
    # ---- all levels in one launch: [L][R][B][12], three distinct extents, a kdiv per level
    kd = [4.0, 1.0, float(np.float32(19.2))]
    kdv = (ctypes.c_float * L)(*kd)
    P_all = torch.full((L, R, B, 12), float("nan"), device=dev)
    E.call("cc_pose_proj_levels", pose_d, K_d, P_all, L, R, B, ctypes.addressof(kdv), STREAM)
    for l in range(L):
        lrb = lambda dt: _proj(pose_flat, K_flat, kd[l], dt).reshape(B, R, 12).transpose(0, 1)
        T.term("levels l=%d kdiv=%g" % (l, kd[l]), P_all[l], lrb(torch.float32), lrb(torch.float64))
    assert torch.equal(P_all[0].cpu(), fwd[4.0].view(B, R, 12).transpose(0, 1)), "cc_pose_proj_levels != cc_pose_proj_fwd at the same kdiv"
    # ---- the adjoint: accumulate flag, both strides
    g = torch.Generator().manual_seed(12)
    gP, pre = torch.randn(N, 12, generator=g), torch.randn(N, 6, generator=g)
    gP_d = gP.to(dev)
    for kdiv in (1.0, 4.0, 32.0):
        g32, g64 = _proj_grad(pose_flat, K_flat, kdiv, gP, torch.float32), _proj_grad(pose_flat, K_flat, kdiv, gP, torch.float64)
        for width in (6, 8):
            for acc in (0, 1):
                buf = torch.full((N, width), -77.0)
                if acc:
                    buf[:, :6] = pre
                buf = buf.to(dev)
                E.call("cc_pose_proj_bwd", gP_d, pose_d.view(N, 6), 6, K_flat_d, buf, width, N, kdiv, acc, STREAM)
                T.term("bwd kdiv=%g gpose_stride=%d accumulate=%d" % (kdiv, width, acc), buf[:, :6],
                       pre + g32 if acc else g32, pre.double() + g64 if acc else g64)
                assert bool((buf[:, 6:] == -77.0).all()), "cc_pose_proj_bwd wrote into the padding of its gradient rows"
        # one reference frame of [B,R,6]: pose rows AND gradient rows 6R floats apart, the other frames' rows stay
        buf = torch.full((B, R, 6), -77.0, device=dev)
        r = 2
        E.call("cc_pose_proj_bwd", gP_d.view(B, R, 12)[:, r].contiguous(), pose_d.data_ptr() + 4 * 6 * r, 6 * R, K_d,
               buf.data_ptr() + 4 * 6 * r, 6 * R, B, kdiv, 0, STREAM)
        T.term("bwd kdiv=%g strides=6R" % kdiv, buf[:, r], g32.reshape(B, R, 6)[:, r], g64.reshape(B, R, 6)[:, r])
        rest = [q for q in range(R) if q != r]
        assert bool((buf[:, rest] == -77.0).all())
    T.done()


def check_rigid_pose_grad_jobs(dev):
    """cc_pose_grad_jobs on synthetic dL/dP partials [B][nb][12], the table built as _PhotoRigidFn builds it: nb = 72 (the lane loop
    wraps, and not a whole number of times), 18 and 1; reference: the float64 sum of the partials per (level, r, b) through the
    float64 adjoint of the projection at that level's kdiv, summed over the levels."""
    import ctypes
    from cc_amd._lib import STREAM
    T = _RigidTerms("grad_jobs")
    L, R, B = 3, 4, 2
    hw = [(96, 192), (48, 96), (5, 7)]
    kd = [1.0, 2.0, float(np.float32(19.2))]
    nb = [(h * w + 255) // 256 for h, w in hw]
    assert nb == [72, 18, 1]
    pose, K = _rigid_poses(B, R, seed=13), _rigid_K(B)
    g = torch.Generator().manual_seed(14)
    # (levels scaled so that each one carries a comparable share of the rotation gradient: K rows 0, 1 are divided by kdiv)
    parts = [torch.randn(B, nb[l], 12, generator=g) * kd[l] for l in range(L) for _ in range(R)]
    parts_d = [p.to(dev) for p in parts]
    pose_d, K_d = pose.to(dev), K.reshape(B, 9).to(dev)
    gpose = torch.full((B, R, 6), float("nan"), device=dev)
    kdv = (ctypes.c_float * L)(*kd)
    jp = LF._Jobs()
    for l in range(L):
        for r in range(R):
            jp.add([parts_d[l * R + r]], *hw[l])
    LF._launch_jobs("cc_pose_grad_jobs", jp, (L, R, B, pose_d, K_d, gpose, ctypes.addressof(kdv), STREAM), R)

    def ref(dt):
        p = _leaf_as(pose, dt)
        tot = 0
        for l in range(L):
            for r in range(R):
                tot = tot + (_proj(p[:, r], K, kd[l], dt) * parts[l * R + r].to(dt).sum(1)).sum()
        return torch.autograd.grad(tot, p)[0]
    T.term("gpose", gpose, ref(torch.float32), ref(torch.float64))
    T.done()


def _rigid_recipe(name, B, R, H, W, seed):
    """-> pose [B,R,6], depth [B,H,W].  'moderate': angles U(-0.4, 0.4), translation N(0, 0.3^2), depth U(0.5, 5.5);
    'behind': angles U(-0.1, 0.1), tz = -2.2 (tx, ty N(0, 0.3^2)), depth in the two bands [0.5, 1.5] and [3.2, 5.2]: about half
    of the pixels end up behind the camera, none close to the Z clamp."""
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g)
    tr = torch.randn(B, R, 3, generator=g) * 0.3
    if name == "moderate":
        ang = (u(B, R, 3) * 2 - 1) * 0.4
        depth = u(B, H, W) * 5 + 0.5
    else:
        ang = (u(B, R, 3) * 2 - 1) * 0.1
        tr[:, :, 2] = -2.2
        depth = torch.where(u(B, H, W) < 0.5, 0.5 + u(B, H, W), 3.2 + 2 * u(B, H, W))
    return torch.cat((tr, ang), 2).float().contiguous(), depth.float().contiguous()


def _rigid_probe(depth, rot, tr, Kinv):
    """float64: the unclamped Z and the normalised coordinates before any rewrite, [B,H,W] each"""
    b, h, w = depth.shape
    cam = G.pixel2cam(depth, Kinv)
    p = cam.view(b, 3, -1)
    if rot is not None:
        p = rot.bmm(p)
    if tr is not None:
        p = p + tr
    grid = G.cam2pixel(cam, rot, tr, None)
    return p[:, 2].view(b, h, w), grid[..., 0], grid[..., 1]


def _rigid_conditions(recipe, Z, xn, yn, full=True):
    """What the recipes promise, asserted on the float64 reference alone.  full: the recipe's own projection (rotation and
    translation); the switched-off variants only have to stay clear of the Z clamp."""
    if recipe == "moderate":
        assert float((Z - 1e-3).abs().min()) >= 0.1, float((Z - 1e-3).abs().min())
        if full:
            inside = float(((xn.abs() <= 1) & (yn.abs() <= 1)).double().mean())
            assert inside >= 0.20, inside
    else:
        assert float(Z.abs().min()) >= 0.2, float(Z.abs().min())
        if full:
            behind = float((Z < 1e-3).double().mean())
            assert 0.30 <= behind <= 0.70, behind


def _excluded_share(tag, excl):
    share = float(excl.double().mean())
    _note("rigid:excluded_share", share)
    print("%-64s excluded %.4f" % (tag, share))
    assert share <= RIGID_MAX_EXCLUDED, (tag, share)
    return share


# seeds at which the recipes meet their conditions (asserted by _rigid_conditions on the float64 reference)
RIGID_SEEDS = {("coords", "moderate"): 2, ("coords", "behind"): 1, ("chain", "moderate"): 4, ("chain", "behind"): 2}


def check_rigid_coords(dev, B=2, H=24, W=40):
    """IW.pixel2cam / IW.cam2pixel (grid and all gradients) and IW.pose2flow (flow, d/d depth, d/dP) at real rotations and with
    points behind the camera, P taken from cc_pose_proj_fwd on the device and handed to all three sides."""
    from cc_amd._lib import engine, STREAM
    T = _RigidTerms("coords")
    _, _, K, Kinv = syn.sample(B, H, W, seed=1)
    for recipe in ("moderate", "behind"):
        pose, depth = _rigid_recipe(recipe, B, 1, H, W, RIGID_SEEDS["coords", recipe])
        P_d = torch.empty(B, 12, device=dev)
        engine().call("cc_pose_proj_fwd", pose[:, 0].contiguous().to(dev), 6, K.reshape(B, 9).to(dev), P_d, B, 1.0, STREAM)
        P = P_d.cpu().view(B, 3, 4)
        for mode, use_rot, use_tr in (("zeros", True, True), ("border", True, True), ("zeros", False, True), ("zeros", True, False)):
            tag = "%s %s%s%s" % (recipe, mode, "" if use_rot else " no-rot", "" if use_tr else " no-tr")
            Z, xn, yn = _rigid_probe(depth.double(), P[:, :, :3].double() if use_rot else None, P[:, :, 3:].double() if use_tr else None,
                                     Kinv.double())
            _rigid_conditions(recipe, Z, xn, yn, full=use_rot and use_tr)
            excl = torch.zeros_like(Z, dtype=torch.bool)
            if mode == "zeros":             # the rewrite decision |xn| = 1, |yn| = 1, measured in pixels
                excl = ((xn.abs() - 1).abs() * (W - 1) / 2 < RIGID_DELTA) | ((yn.abs() - 1).abs() * (H - 1) / 2 < RIGID_DELTA)
            _excluded_share(tag, excl)
            keep = ~excl
            clamped = Z < 1e-3
            wgt = torch.randn(B, H, W, 2, generator=torch.Generator().manual_seed(9))
            wgt[excl] = 0
            sides = {}
            for side, dt in (("dev", torch.float32), ("o32", torch.float32), ("o64", torch.float64)):
                d = dev if side == "dev" else "cpu"
                d_, ki = _leaf_as(depth, dt, d), _leaf_as(Kinv, dt, d)
                rot = _leaf_as(P[:, :, :3].contiguous(), dt, d) if use_rot else None
                tr = _leaf_as(P[:, :, 3:].contiguous(), dt, d) if use_tr else None
                mod = IW if side == "dev" else G
                cam = mod.pixel2cam(d_, ki)
                grid = mod.cam2pixel(cam, rot, tr, mode)
                wrt = {k: t for k, t in (("depth", d_), ("Kinv", ki), ("cam", cam), ("rot", rot), ("tr", tr)) if t is not None}
                gs = torch.autograd.grad((grid * wgt.to(dt).to(d)).sum() + (cam * cam).sum() * 1e-3, list(wrt.values()))
                sides[side] = dict(cam=cam.detach(), grid=grid.detach(), **{"g_" + k: v for k, v in zip(wrt, gs)})
            a, b, c = sides["dev"], sides["o32"], sides["o64"]
            T.term("cam %s" % tag, a["cam"], b["cam"], c["cam"])
            for nm, sel in (("front", keep & ~clamped), ("clamped", keep & clamped)):
                if bool(sel.any()):
                    T.term("grid[%s] %s" % (nm, tag), a["grid"], b["grid"], c["grid"], keep=sel)
            for k in a:
                if k.startswith("g_"):
                    T.term("%s %s" % (k, tag), a[k], b[k], c[k])
        # ---- pose2flow: no rewrite, no clip: nothing to leave out; the Z clamp is taken (recipe 'behind') and stays clear of its edge
        Z, xn, yn = _rigid_probe(depth.double(), P[:, :, :3].double(), P[:, :, 3:].double(), Kinv.double())
        clamped = Z < 1e-3
        gf = torch.randn(B, 2, H, W, generator=torch.Generator().manual_seed(6))
        sides = {}
        for side, dt in (("dev", torch.float32), ("o32", torch.float32), ("o64", torch.float64)):
            d = dev if side == "dev" else "cpu"
            d_ = _leaf_as(depth, dt, d)
            if side == "dev":
                P_ = _leaf_as(P.reshape(B, 12), dt, d)
                f = IW._Pose2FlowFn.apply(d_, P_, Kinv.to(d), 0)
            else:
                P_ = _leaf_as(P, dt)
                f = G.flow_from_projection(d_, P_, Kinv.to(dt))
            gd, gP = torch.autograd.grad(f, [d_, P_], gf.to(dt).to(d))
            sides[side] = dict(flow=f.detach(), g_depth=gd, g_P=gP.reshape(B, 12))
        a, b, c = sides["dev"], sides["o32"], sides["o64"]
        for nm, sel in (("front", ~clamped), ("clamped", clamped)):
            if bool(sel.any()):
                sel2 = sel.unsqueeze(1).expand(B, 2, H, W)
                T.term("flow[%s] %s" % (nm, recipe), a["flow"], b["flow"], c["flow"], keep=sel2)
                T.term("flow g_depth[%s] %s" % (nm, recipe), a["g_depth"], b["g_depth"], c["g_depth"], keep=sel)
        T.term("flow g_P %s" % recipe, a["g_P"], b["g_P"], c["g_P"])
    T.done()


def _pinned_out(Z, xn, yn, H, W, border, ac):
    """float64 unclamped Z and normalised coordinates [B,H,W] -> the pixels within RIGID_DELTA px of a sampling decision: the 'zeros' rewrite
    (|xn| = 1) or the border clip (ix = 0, W - 1), and -- for a coordinate that is neither rewritten nor clipped -- a bilinear tap
    boundary (an integer ix).  ATen's unnormalisation: ix = (xn + 1) / 2 * (W - 1) with align_corners, ((xn + 1) * W - 1) / 2 without."""
    excl = torch.zeros_like(xn, dtype=torch.bool)
    alive = torch.zeros_like(excl)
    for cn, n in ((xn, W), (yn, H)):
        unnorm = (lambda v: (v + 1) / 2 * (n - 1)) if ac else (lambda v: ((v + 1) * n - 1) / 2)
        pix = unnorm(cn)
        if border:
            lo, hi = 0.0, float(n - 1)
            live = (pix > lo) & (pix < hi)
        else:
            lo, hi = float(unnorm(-1.0)), float(unnorm(1.0))
            live = cn.abs() <= 1
        excl |= ((pix - lo).abs() < RIGID_DELTA) | ((pix - hi).abs() < RIGID_DELTA)
        excl |= live & ((pix - pix.round()).abs() < RIGID_DELTA)
        alive |= live
    # a point behind the camera (Z clamped to 1e-3) whose coordinate nevertheless stays inside the image: X / 1e-3 carries the
    # rounding of X (~1e-6) as ~1e-3 px, the size of RIGID_DELTA itself, so its taps cannot be pinned at that distance.  A handful
    # of pixels per map (they count towards the 2 % cap); the clamp itself is held by check_rigid_coords on every such pixel.
    # Consequence: the pinned chain never takes the clamp branch of rigid_backward on a live tap; the warp backward's clamp is covered
    # only through pose2flow (check_rigid_coords: flow g_depth[clamped], flow g_P), which shares rigid_backward with the warps.
    return excl | ((Z < 1e-3) & alive)


def check_rigid_chain(dev, B=2, R=2, C=3):
    """The product's pose-gradient chain cc_pose_proj_levels -> cc_inverse_warp_fwd_jobs -> cc_inverse_warp_bwd_jobs ->
    cc_pose_grad_jobs, called as _PhotoRigidFn calls them (two levels, kdiv 1 and 2), and the single-problem IW.inverse_warp,
    against float64 projection -> pixel2cam -> cam2pixel -> grid_sample under autograd, the sampling decisions pinned."""
    import ctypes
    from cc_amd._lib import engine, STREAM
    E = engine()
    T = _RigidTerms("chain")
    hw, kd = [(24, 40), (12, 20)], [1.0, 2.0]
    S = len(hw)
    px = [h * w for h, w in hw]
    nb = [(n + 255) // 256 for n in px]
    _, refs, K, Kinv = syn.sample(B, *hw[0], seed=1, smooth=3)
    img = [[refs[r], torch.nn.functional.avg_pool2d(refs[r], 2).contiguous()] for r in range(R)]       # [r][s]
    K_s = lambda s, dt: torch.cat((K.to(dt)[:, 0:2] / kd[s], K.to(dt)[:, 2:]), dim=1)
    Kinv_s = lambda s, dt: torch.cat((Kinv.to(dt)[:, :, 0:2] * kd[s], Kinv.to(dt)[:, :, 2:]), dim=2)
    K_d, Kinv_d = K.reshape(B, 9).to(dev), Kinv.to(dev).contiguous()
    Kinv_all = LF._kinv_levels(Kinv_d, kd)
    img_d = [[im.to(dev) for im in per_r] for per_r in img]
    kdv = (ctypes.c_float * S)(*kd)
    for recipe in ("moderate", "behind"):
        pose, d0 = _rigid_recipe(recipe, B, R, *hw[0], RIGID_SEEDS["chain", recipe])
        depth = [d0, d0[:, ::2, ::2].contiguous()]
        pose_d, depth_d = pose.to(dev), [d.to(dev) for d in depth]
        P_all = torch.empty(S, R, B, 12, device=dev)
        E.call("cc_pose_proj_levels", pose_d, K_d, P_all, S, R, B, ctypes.addressof(kdv), STREAM)
        probe = {}
        for s in range(S):
            for r in range(R):
                P64 = G.projection(pose[:, r].double(), K_s(s, torch.float64))
                probe[s, r] = _rigid_probe(depth[s].double(), P64[:, :, :3], P64[:, :, 3:], Kinv_s(s, torch.float64))
                _rigid_conditions(recipe, *probe[s, r])
        for ac in (False, True):
            for pad in ("zeros", "border"):
                border = 1 if pad == "border" else 0
                tag = "%s %s ac=%d" % (recipe, pad, ac)
                go, keep = [], []
                g = torch.Generator().manual_seed(5)
                for s in range(S):
                    for r in range(R):
                        excl = _pinned_out(*probe[s, r], *hw[s], border, ac)
                        _excluded_share("%s level %d ref %d" % (tag, s, r), excl)
                        k3 = (~excl).unsqueeze(1).expand(B, C, *hw[s])
                        keep.append(k3)
                        go.append(torch.randn(B, C, *hw[s], generator=g) * k3)
                go_d = [x.to(dev) for x in go]
                # ---- the device: the four launches of _PhotoRigidFn
                warped = [torch.full((B, C) + hw[s], float("nan"), device=dev) for s in range(S) for _ in range(R)]
                jb = LF._Jobs()
                for s in range(S):
                    for r in range(R):
                        jb.add([img_d[r][s], depth_d[s], P_all[s][r], Kinv_all[s], warped[s * R + r]], *hw[s])
                LF._launch_jobs("cc_inverse_warp_fwd_jobs", jb, (B, C, border, int(ac), STREAM), R)
                gd_all = [torch.full((R, B) + hw[s], float("nan"), device=dev) for s in range(S)]
                gpp = [torch.full((B, nb[s], 12), float("nan"), device=dev) for s in range(S) for _ in range(R)]
                jb, jp = LF._Jobs(), LF._Jobs()
                for s in range(S):
                    for r in range(R):
                        j = s * R + r
                        jb.add([go_d[j], img_d[r][s], depth_d[s], P_all[s][r], Kinv_all[s], LF._off(gd_all[s], r * B * px[s]), gpp[j]],
                               *hw[s])
                        jp.add([gpp[j]], *hw[s])
                LF._launch_jobs("cc_inverse_warp_bwd_jobs", jb, (B, C, border, int(ac), STREAM), R)
                gpose = torch.full((B, R, 6), float("nan"), device=dev)
                LF._launch_jobs("cc_pose_grad_jobs", jp, (S, R, B, pose_d, K_d, gpose, ctypes.addressof(kdv), STREAM), R)
                # ---- the single-problem entry on (level 0, reference frame 0): also the image gradient
                im1, d1, p1 = leaf(img[0][0], dev), leaf(depth[0], dev), leaf(pose[:, 0], dev)
                o1 = IW.inverse_warp(im1, d1, p1, K.to(dev), Kinv_d, padding_mode=pad, align_corners=ac)
                g1 = torch.autograd.grad(o1, [im1, d1, p1], go_d[0])

                # ---- the oracle, fp32 and float64
                def oracle(dt):
                    p, im0 = _leaf_as(pose, dt), _leaf_as(img[0][0], dt)
                    outs, dl, tot = [], [], 0
                    for s in range(S):
                        for r in range(R):
                            dl.append(_leaf_as(depth[s], dt))
                            im = im0 if (s, r) == (0, 0) else img[r][s].to(dt)
                            o = G.inverse_warp(im, dl[-1], p[:, r], K_s(s, dt), Kinv_s(s, dt), padding_mode=pad, align_corners=ac)
                            outs.append(o.detach())
                            tot = tot + (o * go[s * R + r].to(dt)).sum()
                    gr = torch.autograd.grad(tot, [p, im0] + dl)
                    return outs, gr[0], gr[1], gr[2:]
                (w32, gp32, gi32, gd32), (w64, gp64, gi64, gd64) = oracle(torch.float32), oracle(torch.float64)
                for s in range(S):
                    for r in range(R):
                        j = s * R + r
                        T.term("warped %s level %d ref %d" % (tag, s, r), warped[j], w32[j], w64[j], keep=keep[j])
                        T.term("gdepth %s level %d ref %d" % (tag, s, r), gd_all[s][r], gd32[j], gd64[j])
                T.term("gpose %s" % tag, gpose, gp32, gp64)
                # the single problem differentiates level 0, frame 0 alone: its own oracle gradients
                T.term("single:warped %s" % tag, o1, w32[0], w64[0], keep=keep[0])
                T.term("single:gdepth %s" % tag, g1[1], gd32[0], gd64[0])
                T.term("single:gimg %s" % tag, g1[0], gi32, gi64)
                sp = []
                for dt in (torch.float32, torch.float64):
                    p = _leaf_as(pose[:, 0], dt)
                    o = G.inverse_warp(img[0][0].to(dt), depth[0].to(dt), p, K.to(dt), Kinv.to(dt), padding_mode=pad, align_corners=ac)
                    sp.append(torch.autograd.grad((o * go[0].to(dt)).sum(), p)[0])
                T.term("single:gpose %s" % tag, g1[2], sp[0], sp[1])
    T.done()


# ---------------------------------------------------------------------------------------------------------------------
# Every single-call loss-path kernel against the row of a job table that runs the same pixel body (csrc/warp.hip, losses.hip)
SINGLE_JOB_SHAPES = ((8, 26), (20, 53))        # 208 pixels: one ragged 256-pixel piece; 1060: five pieces, odd width
SINGLE_JOB_SEEDS = (3, 4)                      # _rigid_recipe seeds at which 25-75 % of the samples land inside (asserted below)


def check_single_call_equals_job_row(dev):
    """One job-table launch with two rows (SINGLE_JOB_SHAPES, B = 2, C = 3) per *_jobs entry point of the loss path, and the
    single-call entry point on each row's tensors.  Inputs: _rigid_recipe('moderate') poses and depths through cc_pose_proj_fwd, the
    flows are the rigid flows of those poses (a quarter to three quarters of the samples inside the image, asserted), random upstream
    gradients; the warps in all four (align_corners, padding_border) combinations, pose2flow with and without the rewrite.

    Every per-pixel output is torch.equal between the two forms: out, gdepth, gflow, flow, the masks, gpred, gmask, target.

    Reduced outputs are torch.equal exactly where both forms add the same values in the same order (block_sum_256 over one value per
    work-item, a work-item that held a single live pixel):
      cc_edge_smooth_fwd_bwd_jobs, C > 0 (k_edge_smooth_jobs<1>)   every partial sum of both rows; and the loss: k_reduce_add over
      cc_consensus_bce_fwd_bwd_jobs                                  the single calls' partials laid out back to back is the table's sum
      cc_inverse_warp_bwd_jobs (WPPT = 4)                            partial row k of [B][nb][12] where piece k is the only live piece
      cc_edge_smooth_fwd_bwd_jobs, C = 0 (k_edge_smooth_jobs<4>)     of its workgroup: k = 0 of row 0 (nb = 1), k = 4 of row 1 (nb = 5)
      cc_bce_ones_fwd_bwd_jobs                                       never: the single call runs flat over B C H W (256 elements across
                                                                     plane borders), the table form piece by piece of each plane
    Where the layouts differ the layout is asserted: rows k % 4 != 0 of the WPPT / PPT = 4 forms' partial areas are exactly zero,
    every partial area is written over its whole documented extent and not beyond (NaN sentinels).  The values of the sums that are
    added in another order are left to the float64 tests (check_edge_smooth_float64, check_bce_ones_float64,
    check_consensus_bce_float64) and the golden tests.  The table form of edge smoothness runs a second time with the levels' edge
    weights (cc_edge_weights_jobs) in slot 5: the same bits in loss, partials and gpred.
    (The SSIM family: check_ssim_single_call_equals_job_row.)"""
    from cc_amd._lib import engine, STREAM
    E = engine()
    B, C, R = 2, 3, 4
    hw = SINGLE_JOB_SHAPES
    nb = [(h * w + 255) // 256 for h, w in hw]
    assert nb == [1, 5]
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    thresh, wbce, wrig, gscale = 0.5, 0.25, 0.7, 0.75

    rows = []
    for i, (H, W) in enumerate(hw):
        g = torch.Generator().manual_seed(70 + i)
        rn = lambda *s: torch.randn(*s, generator=g)
        ru = lambda *s: torch.rand(*s, generator=g)
        _, refs, K, Kinv = syn.sample(B, H, W, seed=1, smooth=1)
        pose, depth = _rigid_recipe("moderate", B, R, H, W, SINGLE_JOB_SEEDS[i])
        P = torch.empty(B * R, 12, device=dev)
        E.call("cc_pose_proj_fwd", pose.view(B * R, 6).to(dev), 6, K.repeat_interleave(R, 0).reshape(B * R, 9).contiguous().to(dev), P, B * R, 1.0, STREAM)
        d = dict(H=H, W=W, img=refs[0][:, :C].contiguous(), depth=depth, P4=P.cpu().view(B, R, 12).transpose(0, 1).contiguous(),
                 Kinv=Kinv.reshape(B, 9).contiguous(), gout=rn(B, C, H, W), pred=rn(B, C, H, W), mask=torch.sigmoid(rn(B, C, H, W)),
                 exp_mask=torch.sigmoid(rn(B, 4, H, W)), census_b=ru(B, 2, H, W) * 0.7, census_f=ru(B, 2, H, W) * 0.7,
                 tgt_b=(ru(B, 1, H, W) < 0.5).float(), tgt_f=(ru(B, 1, H, W) < 0.5).float(),
                 err_cf=ru(B, 1, H, W), err_cb=ru(B, 1, H, W), err_ff=ru(B, 1, H, W) * 0.5,
                 v_cf=(ru(B, 1, H, W) < 0.5).float(), v_cb=(ru(B, 1, H, W) < 0.5).float())
        d = {k: v.to(dev) if torch.is_tensor(v) else v for k, v in d.items()}
        d["P"] = d["P4"][0].contiguous()
        # the flows of the flow-driven kernels: the rigid flows of frames 0 and 1 (the single call: an input like any other here)
        for k, r in (("flow", 0), ("flow_bw", 1)):
            d[k] = nan(B, 2, H, W)
            E.call("cc_pose2flow_fwd", d["depth"], d["P4"][r].contiguous(), d["Kinv"], d[k], B, H, W, 0, STREAM)
        f = d["flow"].cpu()
        ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
        inside = float(((xs + f[:, 0] >= 0) & (xs + f[:, 0] <= W - 1) & (ys + f[:, 1] >= 0) & (ys + f[:, 1] <= H - 1)).float().mean())
        print("single/jobs row %d (%dx%d): %.3f of the samples inside the image" % (i, H, W, inside))
        assert 0.25 <= inside <= 0.75, (i, inside)
        rows.append(d)

    def jobs(name, slots, *args):
        """ONE launch of `name` over the two rows; slots(d) -> the row's slot list"""
        jb = LF._Jobs()
        for d in rows:
            jb.add(slots(d), d["H"], d["W"])
        E.call(name, jb.pack(), len(jb), *args)

    def eq(tag, a, b):
        assert a.shape == b.shape, (tag, a.shape, b.shape)
        assert not bool(torch.isnan(a).any() | torch.isnan(b).any()), (tag, "an element was not written")
        assert torch.equal(a, b), (tag, "differs in %d elements, max %.3e" % (int((a != b).sum()), float((a - b).abs().max())))

    def outs(shape_of):
        """-> (table form's outputs, single calls' outputs), one NaN-filled tensor per row each"""
        return [nan(*shape_of(d)) for d in rows], [nan(*shape_of(d)) for d in rows]

    def partial_area(per_row):
        """one NaN-filled buffer holding the rows' partial areas back to back (+ a guard element) -> buffer, offsets"""
        offs = [0]
        for n in per_row:
            offs.append(offs[-1] + n)
        return nan(offs[-1] + 1), offs

    def grouped_partials(tag, pj, ps, i):
        """pj, ps [..., nb, N]: the table form's (4 pieces per workgroup) and the single call's partial rows of table row i"""
        for k in range(nb[i]):
            if k % 4:
                assert bool((pj[..., k, :] == 0).all()), (tag, i, k, "not exactly zero")
            elif k + 1 == nb[i]:
                eq("%s partial row %d of table row %d" % (tag, k, i), pj[..., k, :], ps[..., k, :])
            else:
                assert not bool(torch.isnan(pj[..., k, :]).any()), (tag, i, k)

    BCHW = lambda d: (B, C, d["H"], d["W"])
    # ---- the warps
    for ac in (0, 1):
        for border in (0, 1):
            tag = "ac=%d border=%d" % (ac, border)
            oj, os_ = outs(BCHW)
            jobs("cc_inverse_warp_fwd_jobs", lambda d: [d["img"], d["depth"], d["P"], d["Kinv"], oj[rows.index(d)]], B, C, border, ac, STREAM)
            for i, d in enumerate(rows):
                E.call("cc_inverse_warp_fwd", d["img"], d["depth"], d["P"], d["Kinv"], os_[i], B, C, d["H"], d["W"], border, ac, STREAM)
                eq("inverse_warp_fwd out %s row %d" % (tag, i), oj[i], os_[i])
                assert float((oj[i] != 0).float().mean()) > 0.2 or border, (tag, i)

            gj, gs = outs(lambda d: (B, d["H"], d["W"]))
            pj, ps = [nan(B, n, 12) for n in nb], [nan(B, n, 12) for n in nb]
            jobs("cc_inverse_warp_bwd_jobs", lambda d: [d["gout"], d["img"], d["depth"], d["P"], d["Kinv"], gj[rows.index(d)], pj[rows.index(d)]],
                 B, C, border, ac, STREAM)
            for i, d in enumerate(rows):
                E.call("cc_inverse_warp_bwd", d["gout"], d["img"], d["depth"], d["P"], d["Kinv"], gs[i], nan(B, 12), None, ps[i], B, C,
                       d["H"], d["W"], border, ac, STREAM)
                eq("inverse_warp_bwd gdepth %s row %d" % (tag, i), gj[i], gs[i])
                grouped_partials("inverse_warp_bwd %s" % tag, pj[i], ps[i], i)

            oj, os_ = outs(BCHW)
            jobs("cc_flow_warp_fwd_jobs", lambda d: [d["img"], d["flow"], oj[rows.index(d)]], B, C, border, ac, STREAM)
            gj, gs = outs(lambda d: (B, 2, d["H"], d["W"]))
            jobs("cc_flow_warp_bwd_jobs", lambda d: [d["gout"], d["img"], d["flow"], gj[rows.index(d)]], B, C, border, ac, STREAM)
            for i, d in enumerate(rows):
                E.call("cc_flow_warp_fwd", d["img"], d["flow"], os_[i], B, C, d["H"], d["W"], border, ac, STREAM)
                E.call("cc_flow_warp_bwd", d["gout"], d["img"], d["flow"], gs[i], None, B, C, d["H"], d["W"], border, ac, STREAM)
                eq("flow_warp_fwd out %s row %d" % (tag, i), oj[i], os_[i])
                eq("flow_warp_bwd gflow %s row %d" % (tag, i), gj[i], gs[i])

    # ---- rigid flows and the occlusion masks
    for rewrite in (0, 1):
        fj, fs = outs(lambda d: (B, 2, d["H"], d["W"]))
        jobs("cc_pose2flow_fwd_jobs", lambda d: [d["depth"], d["P"], d["Kinv"], fj[rows.index(d)]], B, rewrite, STREAM)
        for i, d in enumerate(rows):
            E.call("cc_pose2flow_fwd", d["depth"], d["P"], d["Kinv"], fs[i], B, d["H"], d["W"], rewrite, STREAM)
            eq("pose2flow_fwd flow rewrite=%d row %d" % (rewrite, i), fj[i], fs[i])
    mj, ms = outs(lambda d: (B, 4, d["H"], d["W"]))
    jobs("cc_rigid_noocc_jobs", lambda d: [d["depth"], d["P4"], d["Kinv"], mj[rows.index(d)]], B, STREAM)
    nj, ns = outs(lambda d: (B, 1, d["H"], d["W"]))
    jobs("cc_flow_noocc_jobs", lambda d: [d["flow_bw"], d["flow"], nj[rows.index(d)]], B, STREAM)
    tj, ts = outs(lambda d: (B, 1, d["H"], d["W"]))
    jobs("cc_consensus_target_jobs", lambda d: [d["err_cf"], d["err_cb"], d["err_ff"], d["v_cf"], d["v_cb"], tj[rows.index(d)]], B, wrig, STREAM)
    for i, d in enumerate(rows):
        H, W = d["H"], d["W"]
        E.call("cc_rigid_noocc_fused", d["depth"], d["P4"], d["Kinv"], ms[i], B, H, W, STREAM)
        E.call("cc_flow_noocc", d["flow_bw"], d["flow"], ns[i], B, H, W, STREAM)
        E.call("cc_consensus_target", d["err_cf"], d["err_cb"], d["err_ff"], d["v_cf"], d["v_cb"], ts[i], wrig, B * H * W, STREAM)
        eq("rigid_noocc masks row %d" % i, mj[i], ms[i])
        eq("flow_noocc mask row %d" % i, nj[i], ns[i])
        eq("consensus target row %d" % i, tj[i], ts[i])
        for nm, m in (("rigid_noocc", ms[i]), ("flow_noocc", ns[i]), ("consensus target", ts[i])):
            assert 0.0 < float(m.mean()) < 1.0, (nm, i, "a constant mask compares nothing")

    def same_loss(tag, loss_j, ps, n):
        """the table's loss = k_reduce_add over the rows' partial sums back to back: the same kernel over the single calls' partials"""
        acc = torch.zeros(1, device=dev)
        E.call("cc_reduce_add", torch.cat([p.reshape(-1) for p in ps]).contiguous(), n, 1.0, acc, STREAM)
        eq(tag, loss_j, acc)

    # ---- edge-aware smoothness: one piece per workgroup (C > 0), four (C = 0: per-job channel counts in slot 4)
    for ppt in (1, 4):
        tag = "edge_smooth<%d>" % ppt
        gj, gs = outs(BCHW)
        part, offs = partial_area([B * C * n for n in nb])
        loss_j = torch.zeros(1, device=dev)
        extra = (lambda d: []) if ppt == 1 else (lambda d: [C, None])
        jobs("cc_edge_smooth_fwd_bwd_jobs", lambda d: [d["img"], d["pred"], gj[rows.index(d)], LF._off(part, offs[rows.index(d)])] + extra(d),
             B, C if ppt == 1 else 0, part, loss_j, gscale, STREAM)
        assert bool(torch.isnan(part[-1])) and not bool(torch.isnan(part[:-1]).any()), (tag, "extent of the partial areas")
        # slot 5 filled: the levels' edge weights from cc_edge_weights_jobs instead of exp() per pixel and plane -- the same bits
        wts = [nan(B, 2, d["H"], d["W"]) for d in rows]
        jobs("cc_edge_weights_jobs", lambda d: [d["img"], wts[rows.index(d)]], B, STREAM)
        gw, _ = outs(BCHW)
        part_w, loss_w = nan(offs[-1] + 1), torch.zeros(1, device=dev)
        jobs("cc_edge_smooth_fwd_bwd_jobs", lambda d: [d["img"], d["pred"], gw[rows.index(d)], LF._off(part_w, offs[rows.index(d)]),
                                                       None if ppt == 1 else C, wts[rows.index(d)]], B, C if ppt == 1 else 0, part_w, loss_w, gscale, STREAM)
        assert bool(torch.isnan(part_w[-1]))
        eq(tag + " partials with slot 5", part_w[:-1], part[:-1])
        eq(tag + " loss with slot 5", loss_w, loss_j)
        for i in range(len(rows)):
            eq("%s gpred with slot 5 row %d" % (tag, i), gw[i], gj[i])
        ps = [nan(B * C, n) for n in nb]
        for i, d in enumerate(rows):
            E.call("cc_edge_smooth_fwd_bwd", d["img"], d["pred"], gs[i], ps[i], torch.zeros(1, device=dev), gscale, B, C, d["H"], d["W"], STREAM)
            eq("%s gpred row %d" % (tag, i), gj[i], gs[i])
            pj = part[offs[i]:offs[i + 1]].view(B * C, nb[i])
            if ppt == 1:
                eq("%s partials row %d" % (tag, i), pj, ps[i])
            else:
                grouped_partials(tag, pj.unsqueeze(-1), ps[i].unsqueeze(-1), i)
        if ppt == 1:
            same_loss(tag + " loss", loss_j, ps, offs[-1])
        assert bool(torch.isfinite(loss_j).all()) and float(loss_j) > 0, (tag, loss_j)

    # ---- explainability BCE: per-pixel gradient only (the sums are laid out differently, see the docstring)
    gj, gs = outs(BCHW)
    part, offs = partial_area([B * C * n for n in nb])
    loss_j = torch.zeros(1, device=dev)
    jobs("cc_bce_ones_fwd_bwd_jobs", lambda d: [d["mask"], gj[rows.index(d)], LF._off(part, offs[rows.index(d)])], B * C, part, loss_j, gscale, STREAM)
    assert bool(torch.isnan(part[-1])) and not bool(torch.isnan(part[:-1]).any()), "bce_ones: one partial sum per 256-pixel piece of a plane"
    for i, d in enumerate(rows):
        n = B * C * d["H"] * d["W"]
        ps = nan((n + 255) // 256 + 1)
        E.call("cc_bce_ones_fwd_bwd", d["mask"], gs[i], ps, torch.zeros(1, device=dev), gscale, n, STREAM)
        assert bool(torch.isnan(ps[-1])) and not bool(torch.isnan(ps[:-1]).any()), "bce_ones: one partial sum per 256 elements"
        eq("bce_ones gmask row %d" % i, gj[i], gs[i])
    assert bool(torch.isfinite(loss_j).all()) and float(loss_j) > 0, loss_j

    # ---- consensus BCE
    gj, gs = outs(lambda d: (B, 4, d["H"], d["W"]))
    part, offs = partial_area([B * n for n in nb])
    loss_j = torch.zeros(1, device=dev)
    jobs("cc_consensus_bce_fwd_bwd_jobs", lambda d: [d["exp_mask"], d["census_b"], d["census_f"], d["tgt_b"], d["tgt_f"], gj[rows.index(d)],
                                                     LF._off(part, offs[rows.index(d)])], B, part, loss_j, thresh, wbce, gscale, STREAM)
    assert bool(torch.isnan(part[-1])) and not bool(torch.isnan(part[:-1]).any()), "consensus_bce: extent of the partial areas"
    ps = [nan(B, n) for n in nb]
    for i, d in enumerate(rows):
        E.call("cc_consensus_bce_fwd_bwd", d["exp_mask"], d["census_b"], d["census_f"], d["tgt_b"], d["tgt_f"], gs[i], ps[i],
               torch.zeros(1, device=dev), thresh, wbce, gscale, B, d["H"], d["W"], STREAM)
        eq("consensus_bce gmask row %d" % i, gj[i], gs[i])
        eq("consensus_bce partials row %d" % i, part[offs[i]:offs[i + 1]].view(B, nb[i]), ps[i])
    same_loss("consensus_bce loss", loss_j, ps, offs[-1])


# ---------------------------------------------------------------------------------------------------------------------
# The SSIM / photometric kernels (csrc/ssim.hip) against float64, per entry point, through the C ABI.
# Bars: the formula of the rigid checks, e_dev <= RIGID_MARGIN * e_32 + floor with e = max|x - f64| / max|f64| over the WHOLE
# tensor (these kernels take no sampling decision: nothing is left out).  Both fp32 sides evaluate the same formula and differ in
# summation order (separable 13 + 13 taps against 169, E[xx] + E[yy] filtered together), fmaf and the 1-ulp v_rcp_f32.
# floor = 2^-23 for per-pixel tensors; for sums of non-negative values k * 2^-24, k = the additions on the longest path from a
# pixel to the result (every intermediate is at most the result, so each addition rounds by at most 2^-24 of it; the handful of
# products and quotients behind the sums are left to the 4 * e_32 part):
#   partials    12   ssim_tile_body: s_rob / s_sl take 4 pixels x 3 channels per work item
#              + 6   block_sum_256: wave_sum, six __shfl_xor levels
#              + 2   block_sum_256: (w0 + w1) + (w2 + w3)                                                        = 20
#   loss_accum  20
#              + 1   k_photo_finalize: one addition per thread (nblk <= 256 here; k_photo_finalize_jobs: nblk <= 64, per lane)
#              + 8   block_sum_256 (the job form: wave_sum, 6)
#              + 1   v0 / n3 + wssim * (v1 / n3)
#              + 1   term += the lambda_oob part
#              + 1   loss_accum[0] += term (the job form: up to 3, acc += terms[j] in job order: 20 + 1 + 6 + 2 + 3) = 32
#   scale_out   4    (1 - wssim) * (n1 / v2) / n3: no inexact addition at all (v2 is a sum of 0 / 1 below 2^24), what is left are
#                    its own four roundings -- fewer than the 4 + 8 + 1 + 8 additions on the path of the count
# (wssim, q and lambda_oob are fp32 values on all three sides: the C ABI takes floats, and 1 - 0.997 in float64 is 7e-6 away from
# 1 - float32(0.997).)
SSIM_K_PARTIALS, SSIM_K_LOSS, SSIM_K_SCALE = 20, 32, 4
SSIM_MIN_COND = 10.0            # min(sigma1_sq + sigma2_sq + C2) / C2 of the float64 reference
SSIM_SHAPES = (
    # TS = 32, HALO = 6 (ssim.hip).  colsafe: ox0 >= 8 and ox0 + 40 <= W
    (2, 40, 72),    # W % 4 == 0: VEC.  3 x 2 tiles, last tile column 8 wide, last tile row 8 high; tile column 1 is colsafe
                    # (32 + 40 <= 72); 12 tiles per job: tile_of's deal-out with q = 1, r = 4
    (2, 33, 74),    # W % 4 == 2: `pairs`, tile column 1 colsafe (32 + 40 <= 74); the second tile row is ONE image row
    (1, 35, 45),    # odd W: the scalar form of load_row16 / load4 / store4 / the adjoint's staging loop; two tile columns
    (2, 8, 26),     # the coarsest level of an 832-wide frame: `pairs`, one tile
    (2, 2, 3),      # smaller than the 6-pixel halo in both directions
)
SSIM_SMOOTH = (0, 1)
SSIM_SEEDS = {}                 # (B, H, W, smooth) -> seed of syn.frames where seed 3 misses SSIM_MIN_COND (none does)
PHOTO_ARGS = tuple(tuple(float(np.float32(v)) for v in a) for a in ((0.997, 0.5, 0.0), (0.5, 0.4, 0.3)))      # wssim, q, lambda_oob
PHOTO_SENTINEL = -77.0
PHOTO_LOSS0 = 2.0 ** -10        # loss_accum before the call (the entry point adds to it): small against the second argument set's
                                # term (~0.5), comparable to the first one's (~5e-3)


def _ssim_cond(x, y):
    import torch.nn.functional as F
    x, y = x.double(), y.double()
    win = L.ssim_window(13, 3).double()
    f = lambda t: F.conv2d(t, win, padding=6, groups=3)
    return float((f(x * x) - f(x).pow(2) + f(y * y) - f(y).pow(2) + 0.03 ** 2).min()) / 0.03 ** 2


def _ssim_frames(B, H, W, smooth):
    """frames 0 and 1 of syn.frames at the recorded seed; the conditioning is asserted on float64"""
    fr = syn.frames(B, H, W, seed=SSIM_SEEDS.get((B, H, W, smooth), 3), n_frames=2, smooth=smooth)
    cond = _ssim_cond(fr[0], fr[1])
    print("ssim inputs %dx%dx%d smooth=%d: min(sigma1_sq + sigma2_sq + C2) / C2 = %.1f" % (B, H, W, smooth, cond))
    assert cond >= SSIM_MIN_COND, (B, H, W, smooth, cond)
    return fr[0], fr[1]


def _at_offset(t, off):
    """t's values in a fresh contiguous tensor that starts `off` floats behind a 16-byte boundary"""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == (4 * off) % 16
    return v


def _photo_inputs(B, H, W, smooth):
    """tgt, warped and the mask tensors of one photometric term.  warped = frame 1 with EXACT zeros in all three channels of a band
    of columns (28..37: across the border of tile columns 0 and 1, where W allows), of the last image row and of three isolated
    pixels; one pixel with only two channels zeroed stays valid.  mask_a = channel 2 of A [B,4,H,W] in {0, 1}, mask_b = channel 1 of
    Bm [B,3,H,W] (sigmoid): with the gradient buffer [B,5,H,W] three different batch strides."""
    x, y = _ssim_frames(B, H, W, smooth)
    warped = y.clone()
    c0, c1 = (28, 38) if W >= 40 else (W // 2, W // 2 + W // 8)
    warped[:, :, :, c0:c1] = 0
    warped[:, :, H - 1] = 0
    for b, r, c in ((0, H // 3, W - 1), (B - 1, H // 2, W // 3), (0, 0, 1)):
        warped[b, :, r, c] = 0
    warped[B - 1, :2, 0, 0] = 0
    assert float(warped[B - 1, 2, 0, 0]) != 0
    valid = L._valid(warped.double())
    assert float(valid[B - 1, 0, 0, 0]) == 1 and float(valid[0, 0, 0, 1]) == 0
    share = float(valid.mean())
    print("photo inputs %dx%dx%d smooth=%d: valid share %.3f" % (B, H, W, smooth, share))
    assert 0.3 <= share <= 0.9, share
    assert _ssim_cond(x, warped) >= SSIM_MIN_COND
    g = torch.Generator().manual_seed(1000 * H + 10 * W + smooth)
    return dict(B=B, H=H, W=W, tgt=x, warped=warped, A=(torch.rand(B, 4, H, W, generator=g) < 0.7).float(),
                Bm=torch.sigmoid(torch.randn(B, 3, H, W, generator=g)), pre=torch.randn(B, 3, H, W, generator=g))


def _photo_call(dev, d, args, compl=0, want_grad=1, use_a=True, use_b=True, off=0, off_b=None, flag0=0.0, bwd=(0,)):
    """cc_ssim_photo_fwd (+ cc_ssim_photo_bwd per entry of `bwd`: its accumulate flag, scale = the device's scale_out) on fresh
    NaN / sentinel-filled outputs; every tensor `off` floats behind a 16-byte boundary (mask_b: off_b).  -> dict of device tensors"""
    from cc_amd._lib import engine, STREAM
    E = engine()
    B, H, W = d["B"], d["H"], d["W"]
    HW = H * W
    wssim, q, lam = args
    put = lambda t, o=off: _at_offset(t.to(dev), o)
    nan = lambda *s: put(torch.full(s, float("nan")))
    tgt, warped = put(d["tgt"]), put(d["warped"])
    A = put(d["A"]) if use_a else None
    Bm = put(d["Bm"], off if off_b is None else off_b) if use_b else None
    G = put(torch.full((B, 5, H, W), PHOTO_SENTINEL)) if (want_grad and use_b) else None
    nblk = int(E.call("cc_ssim_num_blocks", B, H, W))
    assert nblk == B * ((H + 31) // 32) * ((W + 31) // 32)
    part = nan(nblk * 4 + 4)                                        # (+ four guard elements)
    adj = [nan(B, 3, H, W) for _ in range(4)] if want_grad else [None] * 4
    loss, scale, flag = torch.full((1,), PHOTO_LOSS0, device=dev), torch.full((1,), float("nan"), device=dev), torch.full((1,), flag0, device=dev)
    ch = lambda t, c: None if t is None else LF._off(t, c * HW)
    E.call("cc_ssim_photo_fwd", tgt, warped, ch(A, 2), 4 * HW, ch(Bm, 1), 3 * HW, compl, part, adj[0], adj[1], adj[2], adj[3], ch(G, 1), 5 * HW,
           want_grad, wssim, q, lam, loss, scale, flag, SS.gauss13_ptr(), B, H, W, STREAM)
    out = dict(loss=loss, scale=scale, flag=flag, part=part, adj=adj, G=G, gw={}, tgt=tgt, warped=warped)
    for acc in bwd:
        gw = put(d["pre"]) if acc else nan(B, 3, H, W)
        E.call("cc_ssim_photo_bwd", adj[0], adj[1], adj[2], adj[3], tgt, warped, scale, gw, acc, SS.gauss13_ptr(), B, H, W, STREAM)
        out["gw"][acc] = gw
    return out


def _tile_sums(m):
    """[B,C,H,W] -> [B * tiles_y * tiles_x]: sums over the channels and the 32 x 32 tiles, in the single call's tile order"""
    import torch.nn.functional as F
    B, C, H, W = m.shape
    th, tw = (H + 31) // 32, (W + 31) // 32
    p = F.pad(m, (0, tw * 32 - W, 0, th * 32 - H))
    return p.view(B, C, th, 32, tw, 32).sum((1, 3, 5)).reshape(-1)


def _photo_ref(d, args, compl, use_a, use_b, dt):
    """the oracle's photometric term in dtype dt -> term, scale_out, tile sums (robust, ssim loss, valid), d term / d warped,
    d term / d mask_b [B,H,W] (or None)"""
    wssim, q, lam = args
    tgt, w = d["tgt"].to(dt), _leaf_as(d["warped"], dt)
    ma = d["A"][:, 2:3].to(dt) if use_a else None
    mbl = _leaf_as(d["Bm"][:, 1:2], dt) if use_b else None
    masks = ([ma] if use_a else []) + ([1 - mbl if compl else mbl] if use_b else [])
    term = L._photo_term(tgt, w, masks, wssim, q, lam)
    grads = torch.autograd.grad(term, [w] + ([mbl] if use_b else []))
    with torch.no_grad():
        valid = L._valid(w)
        diff, sl = (tgt - w) * valid, 1 - L.ssim(tgt, w) * valid
        for m in masks:
            diff, sl = diff * m, sl * m
        tiles = (_tile_sums(L.robust_l1_per_pix(diff, q=q)), _tile_sums(sl), _tile_sums(valid))
        scale = (1 - wssim) * (valid.nelement() / valid.sum()) / (3 * valid.nelement())
    return dict(term=term.detach(), scale=scale, tiles=tiles, gw=grads[0], gmb=grads[1][:, 0] if use_b else None)


def _photo_sum_terms(T, tag, o, r32, r64):
    """loss_accum, scale_out and the per-tile partials of one cc_ssim_photo_fwd call against float64 (the sums' floors)"""
    T.term("loss_accum " + tag, o["loss"], (PHOTO_LOSS0 + r32["term"]).reshape(1), (PHOTO_LOSS0 + r64["term"]).reshape(1),
           floor=SSIM_K_LOSS * 2.0 ** -24)
    T.term("scale_out " + tag, o["scale"], r32["scale"].reshape(1), r64["scale"].reshape(1), floor=SSIM_K_SCALE * 2.0 ** -24)
    part = o["part"].cpu()
    assert bool(torch.isnan(part[-4:]).all()) and not bool(torch.isnan(part[:-4]).any()), (tag, "extent of the partials")
    part = part[:-4].view(-1, 4)
    for k, nm in ((0, "partials_robust"), (1, "partials_ssim")):
        T.term("%s %s" % (nm, tag), part[:, k], r32["tiles"][k], r64["tiles"][k], floor=SSIM_K_PARTIALS * 2.0 ** -24)
    assert torch.equal(part[:, 2].double(), r64["tiles"][2]), (tag, "the valid count of a tile is exact")
    assert bool((part[:, 3] == 0).all()), (tag, "column 3 of the partials")


def check_ssim_map_float64(dev, shapes=SSIM_SHAPES):
    """cc_ssim_fwd and cc_ssim_bwd (both roles: the second call with the images swapped) against L.ssim in fp32 and float64 and its
    autograd under a random upstream gradient, at every SSIM_SHAPES shape and both smooth values."""
    from cc_amd._lib import engine, STREAM
    E = engine()
    T = _RigidTerms("map", "ssim")
    for (B, H, W) in shapes:
        for smooth in SSIM_SMOOTH:
            tag = "%dx%dx%d smooth=%d" % (B, H, W, smooth)
            x, y = _ssim_frames(B, H, W, smooth)
            go = torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(4))
            ref = {}
            for dt in (torch.float32, torch.float64):
                xl, yl = _leaf_as(x, dt), _leaf_as(y, dt)
                s = L.ssim(xl, yl)
                ref[dt] = (s.detach(),) + torch.autograd.grad(s, [xl, yl], go.to(dt))
            nan = lambda: torch.full((B, 3, H, W), float("nan"), device=dev)
            xd, yd, god, out = x.to(dev), y.to(dev), go.to(dev), nan()
            E.call("cc_ssim_fwd", xd, yd, out, SS.gauss13_ptr(), B, H, W, STREAM)
            T.term("ssim " + tag, out, ref[torch.float32][0], ref[torch.float64][0])
            for k, (a, b) in ((2, (xd, yd)), (1, (yd, xd))):          # the gradient goes to the SECOND image of the call
                sa, sb, sc, g = nan(), nan(), nan(), nan()
                E.call("cc_ssim_bwd", a, b, god, sa, sb, sc, g, SS.gauss13_ptr(), B, H, W, STREAM)
                T.term("g_img%d %s" % (k, tag), g, ref[torch.float32][k], ref[torch.float64][k])
    T.done()


PHOTO_FORMS = ((True, True, 0), (True, True, 1), (False, True, 0), (False, True, 1), (True, False, 0), (False, False, 0))  # mask_a, mask_b, b_complement


def check_ssim_photo_float64(dev, shapes=SSIM_SHAPES):
    """cc_ssim_photo_fwd + cc_ssim_photo_bwd against oracle.losses._photo_term in fp32 and float64: loss_accum (started at
    PHOTO_LOSS0), scale_out, the per-tile partials, gmask * scale_out, the gradient of the warped frame with accumulate 0 and 1;
    three different batch strides, the null-mask forms, b_complement, q = 0.5 and the powf branches; want_grad = 0 with null
    pointers gives the same bits."""
    T = _RigidTerms("photo", "ssim")
    for (B, H, W) in shapes:
        for smooth in SSIM_SMOOTH:
            d = _photo_inputs(B, H, W, smooth)
            for args in PHOTO_ARGS:
                for use_a, use_b, compl in PHOTO_FORMS:
                    tag = "%dx%dx%d smooth=%d wssim=%.3g q=%.2g lambda=%.2g a=%d b=%d compl=%d" % ((B, H, W, smooth) + args + (use_a, use_b, compl))
                    r32, r64 = (_photo_ref(d, args, compl, use_a, use_b, dt) for dt in (torch.float32, torch.float64))
                    o = _photo_call(dev, d, args, compl, 1, use_a, use_b, bwd=(0, 1))
                    assert float(o["flag"]) == 0, tag
                    _photo_sum_terms(T, tag, o, r32, r64)
                    T.term("gwarped " + tag, o["gw"][0], r32["gw"], r64["gw"])
                    T.term("gwarped_accumulate " + tag, o["gw"][1], d["pre"] + r32["gw"], d["pre"].double() + r64["gw"])
                    if use_b:
                        G = o["G"].cpu()
                        assert bool((G[:, [0, 2, 3, 4]] == PHOTO_SENTINEL).all()), (tag, "gmask: a write outside its channel")
                        T.term("gmask " + tag, G[:, 1] * o["scale"].cpu(), r32["gmb"], r64["gmb"])
                    if use_a and use_b and compl == 0:
                        o0 = _photo_call(dev, d, args, compl, 0, use_a, use_b, bwd=())
                        assert bool(torch.isnan(o0["part"][-4:]).all()) and torch.equal(o0["part"][:-4], o["part"][:-4]), (tag, "want_grad = 0", "part")
                        for k in ("loss", "scale", "flag"):
                            assert torch.equal(o0[k], o[k]), (tag, "want_grad = 0", k)
    T.done()


def _err_ref(tgt, warped, wssim, dt):
    tgt, warped = tgt.to(dt), warped.to(dt)
    return (1 - wssim) * L.robust_l1_per_pix(tgt - warped).mean(1, keepdim=True) + wssim * (1 - L.ssim(tgt, warped)).mean(1, keepdim=True)


def check_ssim_err_float64(dev):
    """cc_ssim_err_fwd: the consensus error map against float64, the valid map exactly; the warped frames of the photometric check"""
    from cc_amd._lib import engine, STREAM
    E = engine()
    T = _RigidTerms("err", "ssim")
    for (B, H, W) in SSIM_SHAPES:
        for smooth in SSIM_SMOOTH:
            d = _photo_inputs(B, H, W, smooth)
            for wssim in (PHOTO_ARGS[0][0], PHOTO_ARGS[1][0]):
                tag = "%dx%dx%d smooth=%d wssim=%.3g" % (B, H, W, smooth, wssim)
                err, valid = (torch.full((B, 1, H, W), float("nan"), device=dev) for _ in range(2))
                E.call("cc_ssim_err_fwd", d["tgt"].to(dev), d["warped"].to(dev), err, valid, wssim, SS.gauss13_ptr(), B, H, W, STREAM)
                T.term("err " + tag, err, _err_ref(d["tgt"], d["warped"], wssim, torch.float32), _err_ref(d["tgt"], d["warped"], wssim, torch.float64))
                assert torch.equal(valid.cpu(), L._valid(d["warped"])), (tag, "valid")
    T.done()


def check_ssim_load_paths(dev):
    """The VEC, `pairs` and scalar forms of load_row16 / load4 / store4 / the adjoint's staging loop only move values: at 2x40x72 the
    same data at offsets of 0, 2 and 1 floats from a 16-byte boundary (and mask_b alone one float off: ssim_vec_ok falls back for the
    whole launch) gives the same bits in every output of cc_ssim_fwd, cc_ssim_err_fwd, cc_ssim_photo_fwd and cc_ssim_photo_bwd."""
    from cc_amd._lib import engine, STREAM
    E = engine()
    B, H, W = SSIM_SHAPES[0]
    d = _photo_inputs(B, H, W, 0)

    def same(tag, a, b):
        a, b = a.cpu(), b.cpu()
        assert not bool(torch.isnan(a).any()), (tag, "an element was not written")
        assert torch.equal(a, b), (tag, "differs in %d elements, max %.3e" % (int((a != b).sum()), float((a - b).abs().max())))

    for args in PHOTO_ARGS:
        base = None
        for form, off, off_b in (("vec", 0, None), ("pairs", 2, None), ("scalar", 1, None), ("mask_b + 1", 0, 1)):
            o = _photo_call(dev, d, args, compl=1, off=off, off_b=off_b, bwd=(0, 1))
            assert o["tgt"].data_ptr() % 16 == 4 * off and float(o["flag"]) == 0
            o["part"] = o["part"][:-4]
            if off_b is None:
                nan = lambda *s: _at_offset(torch.full(s, float("nan"), device=dev), off)
                o["map"], o["err"], o["valid"] = nan(B, 3, H, W), nan(B, 1, H, W), nan(B, 1, H, W)
                E.call("cc_ssim_fwd", o["tgt"], o["warped"], o["map"], SS.gauss13_ptr(), B, H, W, STREAM)
                E.call("cc_ssim_err_fwd", o["tgt"], o["warped"], o["err"], o["valid"], args[0], SS.gauss13_ptr(), B, H, W, STREAM)
            if base is None:
                base = o
                continue
            for k in ("loss", "scale", "part", "G") + (("map", "err", "valid") if off_b is None else ()):
                same("%s / vec: %s" % (form, k), o[k], base[k])
            for k in range(4):
                same("%s / vec: adjoint map %d" % (form, k), o["adj"][k], base["adj"][k])
            for acc in (0, 1):
                same("%s / vec: gwarped accumulate=%d" % (form, acc), o["gw"][acc], base["gw"][acc])


SSIM_JOB_SHAPES = ((8, 26), (20, 53), (40, 72))        # 2, 4 and 12 tiles per job at B = 2: 12 = 8 + 4 makes tile_of's deal-out a real permutation


def _photo_jobs(dev, rows, args, compl=1, flag0=0.0):
    """ONE cc_ssim_photo_fwd_jobs / cc_ssim_photo_bwd_jobs / cc_ssim_err_fwd_jobs launch each over `rows` (_photo_inputs dicts),
    NaN / sentinel-filled outputs with guard elements -> dict of device tensors (lists: one entry per row)"""
    from cc_amd._lib import engine, STREAM
    E = engine()
    B = rows[0]["B"]
    wssim, q, lam = args
    n = len(rows)
    nan = lambda k: torch.full((k,), float("nan"), device=dev)
    nblk = [B * ((d["H"] + 31) // 32) * ((d["W"] + 31) // 32) for d in rows]
    offs = [0]
    for k in nblk:
        offs.append(offs[-1] + 4 * k)
    part = nan(offs[-1] + 4)
    px = [B * 3 * d["H"] * d["W"] for d in rows]
    dv = [{k: d[k].to(dev) for k in ("tgt", "warped", "A", "Bm")} for d in rows]
    adj = [nan(4 * p + 1) for p in px]
    G = [torch.full((B, 5, d["H"], d["W"]), PHOTO_SENTINEL, device=dev) for d in rows]
    gw, err, valid = [nan(p + 1) for p in px], [nan(p // 3 + 1) for p in px], [nan(p // 3 + 1) for p in px]
    loss, scale, flag = torch.full((1,), PHOTO_LOSS0, device=dev), nan(n + 1), torch.full((1,), flag0, device=dev)
    jb = LF._Jobs()
    for i, d in enumerate(rows):
        HW = d["H"] * d["W"]
        jb.add([dv[i]["tgt"], dv[i]["warped"], LF._off(dv[i]["A"], 2 * HW), LF._off(dv[i]["Bm"], HW), LF._off(G[i], HW), adj[i],
                LF._off(part, offs[i]), 4 | (3 << 8) | (5 << 16)], d["H"], d["W"])
    E.call("cc_ssim_photo_fwd_jobs", jb.pack(), n, B, compl, 1, wssim, q, lam, loss, scale, flag, SS.gauss13_ptr(), STREAM)
    jb = LF._Jobs()
    for i, d in enumerate(rows):
        jb.add([adj[i], dv[i]["tgt"], dv[i]["warped"], LF._off(scale, i), gw[i]], d["H"], d["W"])
    E.call("cc_ssim_photo_bwd_jobs", jb.pack(), n, B, SS.gauss13_ptr(), STREAM)
    jb = LF._Jobs()
    for i, d in enumerate(rows):
        jb.add([dv[i]["tgt"], dv[i]["warped"], err[i], valid[i]], d["H"], d["W"])
    E.call("cc_ssim_err_fwd_jobs", jb.pack(), n, B, wssim, SS.gauss13_ptr(), STREAM)
    return dict(loss=loss, scale=scale, flag=flag, part=part, offs=offs, adj=adj, G=G, gw=gw, err=err, valid=valid, dv=dv)


def check_ssim_single_call_equals_job_row(dev):
    """check_single_call_equals_job_row for the SSIM family: one launch of cc_ssim_photo_fwd_jobs, cc_ssim_photo_bwd_jobs and
    cc_ssim_err_fwd_jobs over three rows (SSIM_JOB_SHAPES, B = 2; slot 7 = three different batch strides) and the single calls on
    each row's tensors.  torch.equal: the four adjoint maps, gmask (with the untouched channels around it), gwarped (both forms
    scaled by the table's scale_out[j]), err, valid and every row's partials (`local` of tile_of is the single call's tile index,
    block_sum_256 is the same).  scale_out[j] and the loss come from another reduction (one wave per job, the terms added in job
    order): held to the float64 bars of check_ssim_photo_float64.  Every area is written over its whole extent (no NaN left) and
    not beyond (guard elements, sentinels)."""
    from cc_amd._lib import engine, STREAM
    E = engine()
    T = _RigidTerms("jobs", "ssim")
    B = 2
    rows = [_photo_inputs(B, H, W, 0) for H, W in SSIM_JOB_SHAPES]

    def eq(tag, a, b):
        assert a.shape == b.shape, (tag, a.shape, b.shape)
        assert not bool(torch.isnan(a).any() | torch.isnan(b).any()), (tag, "an element was not written")
        assert torch.equal(a, b), (tag, "differs in %d elements, max %.3e" % (int((a != b).sum()), float((a - b).abs().max())))

    def body(tag, t):
        assert bool(torch.isnan(t[-1])), (tag, "a write behind the documented extent")
        return t[:-1]

    for args in PHOTO_ARGS:
        for compl in (0, 1):
            J = _photo_jobs(dev, rows, args, compl)
            assert float(J["flag"]) == 0
            assert bool(torch.isnan(J["part"][-4:]).all()) and bool(torch.isnan(J["scale"][-1])), "extent of the partial areas / of scale_out"
            r32 = [_photo_ref(d, args, compl, True, True, torch.float32) for d in rows]
            r64 = [_photo_ref(d, args, compl, True, True, torch.float64) for d in rows]
            for i, d in enumerate(rows):
                tag = "%dx%d wssim=%.3g q=%.2g compl=%d row %d" % (d["H"], d["W"], args[0], args[1], compl, i)
                H, W = d["H"], d["W"]
                S = _photo_call(dev, d, args, compl, bwd=())
                eq("adjoint maps " + tag, body("adjoint maps " + tag, J["adj"][i]), torch.cat([a.reshape(-1) for a in S["adj"]]))
                eq("gmask " + tag, J["G"][i], S["G"])
                assert bool((J["G"][i][:, [0, 2, 3, 4]] == PHOTO_SENTINEL).all()), (tag, "gmask: a write outside its channel")
                eq("partials " + tag, J["part"][J["offs"][i]:J["offs"][i + 1]], S["part"][:-4])
                gw = torch.full((B, 3, H, W), float("nan"), device=dev)
                E.call("cc_ssim_photo_bwd", S["adj"][0], S["adj"][1], S["adj"][2], S["adj"][3], S["tgt"], S["warped"], LF._off(J["scale"], i), gw, 0,
                       SS.gauss13_ptr(), B, H, W, STREAM)
                eq("gwarped " + tag, body("gwarped " + tag, J["gw"][i]).view(B, 3, H, W), gw)
                err, valid = (torch.full((B, 1, H, W), float("nan"), device=dev) for _ in range(2))
                E.call("cc_ssim_err_fwd", S["tgt"], S["warped"], err, valid, args[0], SS.gauss13_ptr(), B, H, W, STREAM)
                eq("err " + tag, body("err " + tag, J["err"][i]).view(B, 1, H, W), err)
                eq("valid " + tag, body("valid " + tag, J["valid"][i]).view(B, 1, H, W), valid)
                T.term("scale_out " + tag, J["scale"][i:i + 1], r32[i]["scale"].reshape(1), r64[i]["scale"].reshape(1), floor=SSIM_K_SCALE * 2.0 ** -24)
                T.term("gwarped " + tag, gw, r32[i]["gw"], r64[i]["gw"])
            tag = "wssim=%.3g q=%.2g compl=%d" % (args[0], args[1], compl)
            T.term("loss_accum " + tag, J["loss"], (PHOTO_LOSS0 + sum(r["term"] for r in r32)).reshape(1),
                   (PHOTO_LOSS0 + sum(r["term"] for r in r64)).reshape(1), floor=SSIM_K_LOSS * 2.0 ** -24)
    T.done()


def check_ssim_nan_flag(dev):
    """The NaN flag of k_photo_finalize / k_photo_finalize_jobs (the deferred form of the reference's `assert loss == loss`) on real
    input, single call and job table, on the 40x72 row.  (These kernels form no address from data: a non-finite pixel moves no
    access.)"""
    B = 2
    args = PHOTO_ARGS[0]
    rows = [_photo_inputs(B, H, W, 0) for H, W in SSIM_JOB_SHAPES]
    d = rows[-1]
    H, W = d["H"], d["W"]
    ref = lambda e: float(L._photo_term(e["tgt"], e["warped"], [e["A"][:, 2:3], e["Bm"][:, 1:2]], *args))
    clean = _photo_call(dev, d, args, bwd=())
    clean_j = _photo_jobs(dev, rows, args, 0)
    for o, scale in ((clean, clean["scale"]), (clean_j, clean_j["scale"][:-1])):          # (the table's scale_out ends in a guard element)
        assert float(o["flag"]) == 0 and bool(torch.isfinite(o["loss"]).all()) and bool(torch.isfinite(scale).all())
    assert np.isfinite(ref(d))
    # a flag that is already raised is not cleared by a clean call
    assert float(_photo_call(dev, d, args, bwd=(), flag0=1.0)["flag"]) == 1
    assert float(_photo_jobs(dev, rows, args, 0, flag0=1.0)["flag"]) == 1
    bad_tgt = dict(d, tgt=d["tgt"].clone())
    bad_tgt["tgt"][B - 1, 2, H - 1, W - 1] = float("nan")          # the last pixel of the ragged corner tile
    bad_w = dict(d, warped=d["warped"].clone())
    assert float(L._valid(d["warped"])[0, 0, 5, 5]) == 1
    bad_w["warped"][0, 1, 5, 5] = float("nan")                     # one channel: NaN != 0, the pixel counts as valid
    for tag, e in (("NaN in tgt", bad_tgt), ("NaN in warped", bad_w)):
        assert np.isnan(ref(e)), (tag, "the fp32 oracle's term")
        o = _photo_call(dev, e, args, bwd=())
        assert float(o["flag"]) == 1 and bool(torch.isnan(o["loss"]).all()), (tag, "single call", o["flag"], o["loss"])
        assert torch.equal(o["scale"], clean["scale"]), tag          # (the valid count does not see the NaN)
        o = _photo_jobs(dev, rows[:-1] + [e], args, 0)
        assert float(o["flag"]) == 1 and bool(torch.isnan(o["loss"]).all()), (tag, "job table", o["flag"], o["loss"])
        assert bool(torch.isfinite(o["scale"][:-1]).all()) and torch.equal(o["scale"][:-1], clean_j["scale"][:-1]), (tag, "scale_out of the rows")
    # warped all zeros: oob = N / 0 = inf and the term is inf on both sides; inf == inf, so the reference's assertion passes too
    zero = dict(d, warped=torch.zeros_like(d["warped"]))
    assert ref(zero) == float("inf")
    for o in (_photo_call(dev, zero, args, bwd=()), _photo_jobs(dev, rows[:-1] + [zero], args, 0)):
        assert float(o["flag"]) == 0 and float(o["loss"]) == float("inf"), (o["flag"], o["loss"])


# ---------------------------------------------------------------------------------------------------------------------
# The rest of csrc/losses.hip against float64, per entry point, through the C ABI: the two smoothness kernels, the two BCE kernels,
# the consensus target, the occlusion masks, the element-wise job kernel, k_reduce_add and the pyramid.
# Bars: e_dev <= RIGID_MARGIN * e_32 + floor with e = max|x - f64| / max|f64|, the references are oracle.losses in fp32 and float64.
# floor = 2^-23 for per-pixel tensors; for sums of non-negative terms (asserted on float64) k * 2^-24, k = the additions on the
# longest path from a pixel to the result:
#   block_sum_256       6   wave_sum: six __shfl_xor levels
#                     + 2   (w0 + w1) + (w2 + w3)                                                                = LOSSK_K_BLOCK = 8
#   partials, per kernel (LOSSK_K): the additions of a work-item into `part`, then block_sum_256
#     edge1           2 + 8   edge_smooth_px: `part +=` the H-direction term, `part +=` the W-direction term (k_edge_smooth, jobs<1>)
#     edge4           8 + 8   k_edge_smooth_jobs<4>: four pixels per work-item
#     smooth2         3 + 8   k_smooth2: dx2, dy2, dxy
#     bce_ones        0 + 8   one term per work-item
#     consensus_bce   5 + 8   consensus_bce_px: w1 * .. + w0 * .. inside a channel's term, `part -=` for four channels
#   loss_accum = the kernel's k + _k_reduce(n) for n partial sums:
#     k_reduce_add    ceil(n / 256)   a work-item adds partials[tid], [tid + 256], ... in index order
#                   + 8               block_sum_256
#                   + 1               accum[0] += coef * v   (cc_reduce_add on its own, coef != 1: + 1 for the product)
# Scalars of the ABI (thresh, wbce, wrig, gscale, weight, coef) are fp32 values on all three sides.
# Decision outputs (the occlusion masks, the consensus target) are exactly the float64 decision wherever float64's margin
# |lhs - rhs| / max(|lhs|, |rhs|) exceeds LOSSK_DELTA; the elements inside are left out on all sides (at most RIGID_MAX_EXCLUDED).
# LOSSK_DELTA = 1e-5: either side of such a comparison is at most eight fp32 operations on values no larger than the larger side
# (8 * 2^-24 = 5e-7 of it), twenty times less.
LOSSK_SHAPES = ((8, 26), (20, 53), (3, 3), (2, 3), (2, 2))       # one ragged piece; five pieces, odd width; every pixel a border pixel
LOSSK_B = 2
LOSSK_GSCALE = float(np.float32(0.7))
LOSSK_DELTA = 1e-5
LOSSK_K_BLOCK = 8
LOSSK_K = dict(edge1=2 + LOSSK_K_BLOCK, edge4=8 + LOSSK_K_BLOCK, smooth2=3 + LOSSK_K_BLOCK, bce_ones=0 + LOSSK_K_BLOCK,
               consensus_bce=5 + LOSSK_K_BLOCK)
# seeds at which the inputs meet the conditions the checks assert on the float64 reference (tie shares, class shares, zero second
# differences); every other (check, H, W) takes seed 0
LOSSK_SEEDS = {("smooth2", 3, 3): 3, ("smooth2", 2, 2): 2, ("decisions", 2, 2): 1}
F32, F64 = torch.float32, torch.float64


def _k_reduce(n):
    return (n + 255) // 256 + LOSSK_K_BLOCK + 1


def _lossk_gen(check, H, W, extra=0):
    seed = LOSSK_SEEDS.get((check, H, W), 0)
    return torch.Generator().manual_seed(100003 * seed + 1009 * H + 13 * W + extra)


def _piece_sums(m):
    """per-pixel terms [..., H, W] -> [planes, nb]: the sums over the 256-pixel pieces of every plane (leading dimensions flattened)"""
    import torch.nn.functional as F
    HW = m.shape[-2] * m.shape[-1]
    nb = (HW + 255) // 256
    return F.pad(m.reshape(-1, HW), (0, nb * 256 - HW)).view(-1, nb, 256).sum(2)


def _group4(ps):
    """[planes, nb] -> the layout of a four-pieces-per-workgroup kernel: piece 4k holds the sum of pieces 4k .. 4k + 3, the others 0"""
    out = torch.zeros_like(ps)
    for k in range(0, ps.shape[1], 4):
        out[:, k] = ps[:, k:k + 4].sum(1)
    return out


def _guarded(tag, t):
    """a NaN-filled area with one guard element behind it: written over its whole extent and not beyond -> the area"""
    assert bool(torch.isnan(t[-1])), (tag, "a write behind the documented extent")
    assert not bool(torch.isnan(t[:-1]).any()), (tag, "an element of the documented extent was not written")
    return t[:-1]


def _lossk_jobs(name, rows, *args):
    """ONE launch of the *_jobs entry point `name`; rows: (slots, H, W)"""
    from cc_amd._lib import engine
    jb = LF._Jobs()
    for slots, H, W in rows:
        jb.add(slots, H, W)
    engine().call(name, jb.pack(), len(jb), *args)


def _offsets(sizes):
    offs = [0]
    for n in sizes:
        offs.append(offs[-1] + n)
    return offs


# ------------------------------------------------------------------ edge-aware smoothness
def _tied_pred(check, C, H, W, planted):
    """randn [B,C,H,W]; planted: exact ties with the left neighbour and with the upper neighbour (a tenth of the pixels each, maps
    wider / higher than 3) and at two corners (the corner pixel's two neighbours take its value)"""
    g = _lossk_gen(check, H, W, extra=7 * C + (1 if planted else 0))
    p = torch.randn(LOSSK_B, C, H, W, generator=g)
    if planted:
        mh, mv = torch.rand(LOSSK_B, C, H, W, generator=g) < 0.1, torch.rand(LOSSK_B, C, H, W, generator=g) < 0.1
        if W > 3:
            for x in range(1, W):
                p[..., x] = torch.where(mh[..., x], p[..., x - 1], p[..., x])
        if H > 3:
            for y in range(1, H):
                p[..., y, :] = torch.where(mv[..., y, :], p[..., y - 1, :], p[..., y, :])
        p[..., 0, 1] = p[..., 0, 0]
        p[..., 1, 0] = p[..., 0, 0]
        p[..., H - 1, W - 2] = p[..., H - 1, W - 1]
        p[..., H - 2, W - 1] = p[..., H - 1, W - 1]
    return p.contiguous()


def _tie_share(p):
    dh, dw = L._grad_h(p), L._grad_w(p)
    return float(((dh == 0).sum() + (dw == 0).sum()).double() / (dh.numel() + dw.numel()))


def _edge_ref(img, pred, dt):
    """L.edge_aware_smoothness_loss of one level in dtype dt (the image is the level's: its pooling is the identity) -> loss,
    d loss / d pred * LOSSK_GSCALE, the per-pixel terms [B,C,H,W] (both directions, anchored at the pixel), the weights [B,2,H,W]"""
    import torch.nn.functional as F
    im, p = img.to(dt), _leaf_as(pred, dt)
    loss = L.edge_aware_smoothness_loss(im, [p])
    g = torch.autograd.grad(loss, p)[0] * LOSSK_GSCALE
    with torch.no_grad():
        wx = torch.exp(-torch.mean(torch.abs(L._grad_h(im)), 1, keepdim=True))
        wy = torch.exp(-torch.mean(torch.abs(L._grad_w(im)), 1, keepdim=True))
        tx, ty = torch.abs(L._grad_h(p)) * wx, torch.abs(L._grad_w(p)) * wy
        terms = F.pad(tx / tx.numel(), (0, 0, 0, 1)) + F.pad(ty / ty.numel(), (0, 1, 0, 0))
        wts = torch.cat((F.pad(wy, (0, 1, 0, 0)), F.pad(wx, (0, 0, 0, 1))), 1)
    return dict(loss=loss.detach(), g=g, terms=terms, wts=wts)


EDGE_C0_ROWS = (((8, 26), 1), ((20, 53), 2), ((3, 3), 4), ((2, 3), 1), ((2, 2), 2), ((20, 53), 4))      # (level, channels in slot 4)


def check_edge_smooth_float64(dev, planted=True):
    """cc_edge_smooth_fwd_bwd, cc_edge_smooth_fwd_bwd_jobs with C = 3 and with C = 0 (EDGE_C0_ROWS: 1 / 2 / 4 channels in slot 4, four
    pieces per workgroup) and cc_edge_weights_jobs at LOSSK_SHAPES against L.edge_aware_smoothness_loss in fp32 and float64: the
    loss, every partial area (NaN fill + guard element), gpred under gscale = 0.7, the weights (exactly 0 in the last column / row).
    Either table form with the weights in slot 5 is torch.equal to slot 5 null; the single call refuses a level of one row or one
    column (the table form takes it and returns a finite number where the reference's mean of an empty tensor is NaN).  planted: `pred` holds exact ties (more than 5 % of
    the neighbour pairs, asserted), where sgn(0) = 0 is the reference's d|x|/dx; otherwise none (asserted)."""
    from cc_amd._lib import engine, STREAM
    E = engine()
    B = LOSSK_B
    check = "edge_ties" if planted else "edge_random"
    T = _RigidTerms(check, "lossk")
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    g0 = {hw: _lossk_gen("edge_img", *hw) for hw in LOSSK_SHAPES}
    imgs = {hw: torch.rand(B, 3, hw[0], hw[1], generator=g0[hw]) * 2 - 1 for hw in LOSSK_SHAPES}
    img_d = {hw: im.to(dev) for hw, im in imgs.items()}
    cache = {}

    def case(hw, C):
        if (hw, C) not in cache:
            pred = _tied_pred(check, C, hw[0], hw[1], planted)
            share = _tie_share(pred)
            print("%s %dx%d C=%d: tie share %.3f" % (check, hw[0], hw[1], C, share))
            assert (share > 0.05) if planted else (share == 0), (hw, C, share)
            r32, r64 = _edge_ref(imgs[hw], pred, F32), _edge_ref(imgs[hw], pred, F64)
            assert float(r64["terms"].min()) >= 0
            cache[(hw, C)] = dict(pred=pred.to(dev), r32=r32, r64=r64)
        return cache[(hw, C)]

    # ---- the weights of every level in one launch
    wt = {hw: nan(B * 2 * hw[0] * hw[1] + 1) for hw in LOSSK_SHAPES}
    _lossk_jobs("cc_edge_weights_jobs", [([img_d[hw], wt[hw]], hw[0], hw[1]) for hw in LOSSK_SHAPES], B, STREAM)
    for hw in LOSSK_SHAPES:
        tag = "%dx%d" % hw
        w = _guarded("weights " + tag, wt[hw]).view(B, 2, hw[0], hw[1]).cpu()
        assert bool((w[:, 0, :, -1] == 0).all()) and bool((w[:, 1, -1, :] == 0).all()), (tag, "weights beyond the last column / row")
        T.term("weights " + tag, w, case(hw, 3)["r32"]["wts"], case(hw, 3)["r64"]["wts"])

    def compare(form, ppt, rows, part, offs, gp, loss):
        ref = [case(hw, Cj) for hw, Cj in rows]
        _guarded(form + " partials", part)
        k = LOSSK_K["edge%d" % ppt]
        T.term("loss_%s" % form, loss, sum(r["r32"]["loss"] for r in ref).reshape(1), sum(r["r64"]["loss"] for r in ref).reshape(1),
               floor=(k + _k_reduce(offs[-1])) * 2.0 ** -24)
        grp = _group4 if ppt == 4 else (lambda x: x)
        for i, ((hw, Cj), r) in enumerate(zip(rows, ref)):
            tag = "%dx%d C=%d" % (hw[0], hw[1], Cj)
            pj = part[offs[i]:offs[i + 1]].view(B * Cj, -1)
            T.term("partials_%s %s" % (form, tag), pj, grp(_piece_sums(r["r32"]["terms"])), grp(_piece_sums(r["r64"]["terms"])), floor=k * 2.0 ** -24)
            T.term("gpred_%s %s" % (form, tag), gp[i], r["r32"]["g"], r["r64"]["g"])

    def table(rows, C, with_weights):
        offs = _offsets([B * Cj * ((hw[0] * hw[1] + 255) // 256) for hw, Cj in rows])
        part, loss = nan(offs[-1] + 1), torch.zeros(1, device=dev)
        gp = [nan(B, Cj, hw[0], hw[1]) for hw, Cj in rows]
        _lossk_jobs("cc_edge_smooth_fwd_bwd_jobs",
                    [([img_d[hw], case(hw, Cj)["pred"], gp[i], LF._off(part, offs[i]), None if C else Cj, wt[hw] if with_weights else None],
                      hw[0], hw[1]) for i, (hw, Cj) in enumerate(rows)], B, C, part, loss, LOSSK_GSCALE, STREAM)
        return part, offs, gp, loss

    # ---- the single call per level
    for hw in LOSSK_SHAPES:
        nb = (hw[0] * hw[1] + 255) // 256
        part, loss, gp = nan(B * 3 * nb + 1), torch.zeros(1, device=dev), nan(B, 3, hw[0], hw[1])
        E.call("cc_edge_smooth_fwd_bwd", img_d[hw], case(hw, 3)["pred"], gp, part, loss, LOSSK_GSCALE, B, 3, hw[0], hw[1], STREAM)
        compare("single", 1, [(hw, 3)], part, [0, B * 3 * nb], [gp], loss)
    # a level of one row or one column (the reference's loss is NaN there: the mean of an empty tensor): the single call refuses it
    for (H, W) in ((1, 5), (4, 1)):
        g = torch.Generator().manual_seed(31)
        img, pred = torch.rand(B, 3, H, W, generator=g) * 2 - 1, torch.randn(B, 3, H, W, generator=g)
        assert bool(torch.isnan(L.edge_aware_smoothness_loss(img, [pred])))
        with pytest.raises(RuntimeError):
            E.call("cc_edge_smooth_fwd_bwd", img.to(dev), pred.to(dev), nan(B, 3, H, W), nan(B * 3 + 1), torch.zeros(1, device=dev), LOSSK_GSCALE, B, 3, H, W, STREAM)
    # ---- the table forms, slot 5 null and filled
    for form, ppt, rows, C in (("jobs1", 1, [(hw, 3) for hw in LOSSK_SHAPES], 3), ("jobs4", 4, list(EDGE_C0_ROWS), 0)):
        part, offs, gp, loss = table(rows, C, False)
        compare(form, ppt, rows, part, offs, gp, loss)
        part_w, _, gp_w, loss_w = table(rows, C, True)
        assert torch.equal(loss_w, loss) and torch.equal(_guarded(form + " partials (slot 5)", part_w), part[:-1]), (form, "slot 5: loss, partials")
        for a, b in zip(gp_w, gp):
            assert not bool(torch.isnan(a).any()) and torch.equal(a, b), (form, "slot 5: gpred")
    T.done()


# ------------------------------------------------------------------ second-order smoothness
SMOOTH2_WEIGHTS = tuple(float(np.float32(v)) for v in (1.0, 1.0 / 2.3 ** 2))


def check_smooth2_float64(dev):
    """cc_smooth2_fwd_bwd (no table form) against weight * L.smooth_loss in fp32 and float64 at weight = 1 and 1 / 2.3^2, gscale =
    0.7: loss and gpred, the extent of the partials.  pred is quantised to multiples of 1/4 so that more than 5 % of the second
    differences of each stencil are exactly 0 (asserted): sgn(0) = 0 is the reference's gradient there.  H < 3 or W < 3: NaN on
    both sides, the gradient of the non-empty stencils."""
    from cc_amd._lib import engine, STREAM
    E = engine()
    B, C = LOSSK_B, 3
    T = _RigidTerms("smooth2", "lossk")
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    for (H, W) in LOSSK_SHAPES:
        pred = torch.round(torch.randn(B, C, H, W, generator=_lossk_gen("smooth2", H, W)) * 2) / 4
        dx, dy = pred[..., 1:] - pred[..., :-1], pred[..., 1:, :] - pred[..., :-1, :]
        for nm, d in (("dx2", dx[..., 1:] - dx[..., :-1]), ("dxdy", dx[..., 1:, :] - dx[..., :-1, :]), ("dy2", dy[..., 1:, :] - dy[..., :-1, :])):
            if d.numel():
                share = float((d == 0).double().mean())
                print("smooth2 %dx%d: share of exact zeros in %s %.3f" % (H, W, nm, share))
                assert share > 0.05, (H, W, nm, share)
        degenerate = H < 3 or W < 3
        nb = (H * W + 255) // 256
        for weight in SMOOTH2_WEIGHTS:
            tag = "%dx%d weight=%.3g" % (H, W, weight)
            ref = {}
            for dt in (F32, F64):
                p = _leaf_as(pred, dt)
                loss = L.smooth_loss([p]) * weight
                ref[dt] = (loss.detach(), torch.autograd.grad(loss, p)[0] * LOSSK_GSCALE)
                assert bool(torch.isnan(loss)) == degenerate and (degenerate or float(loss) >= 0), (tag, loss)
            part, loss, gp = nan(B * C * nb + 1), torch.zeros(1, device=dev), nan(B, C, H, W)
            E.call("cc_smooth2_fwd_bwd", pred.to(dev), gp, part, loss, weight, LOSSK_GSCALE, B * C, H, W, STREAM)
            _guarded("partials " + tag, part)
            if degenerate:
                assert bool(torch.isnan(loss).all()), (tag, loss)
            else:
                T.term("loss " + tag, loss, ref[F32][0].reshape(1), ref[F64][0].reshape(1), floor=(LOSSK_K["smooth2"] + _k_reduce(B * C * nb)) * 2.0 ** -24)
            T.term("gpred " + tag, gp, ref[F32][1], ref[F64][1])
    T.done()


# ------------------------------------------------------------------ BCE against ones
BCE_PLANTED = (0.0, 1.0, 1e-45, 1e-30, 1e-13, 2.0 ** -24, 1.0 - 2.0 ** -24)       # the -100 clamp of the log, the 1e-12 clamp of the gradient


def _bce_ones_ref(mask, dt):
    """L.explainability_loss of one level in dtype dt -> loss, d loss / d mask * LOSSK_GSCALE, the per-element terms"""
    import torch.nn.functional as F
    m = _leaf_as(mask, dt)
    loss = L.explainability_loss([m])
    g = torch.autograd.grad(loss, m)[0] * LOSSK_GSCALE
    with torch.no_grad():
        terms = F.binary_cross_entropy(m, torch.ones_like(m), reduction="none") / m.numel()
    return dict(loss=loss.detach(), g=g, terms=terms.detach())


def check_bce_ones_float64(dev, planted=True):
    """cc_bce_ones_fwd_bwd (flat over B C H W) and cc_bce_ones_fwd_bwd_jobs (piece by piece of each plane) at LOSSK_SHAPES, C = 4,
    against L.explainability_loss (F.binary_cross_entropy) in fp32 and float64: loss, partials, gmask under gscale = 0.7.  planted:
    BCE_PLANTED values among the sigmoid ones; each planted element of gmask is a term of its own, the ordinary elements another
    (one planted gradient is -1e12 / n beside -1 / n)."""
    from cc_amd._lib import engine, STREAM
    E = engine()
    B, C = LOSSK_B, 4
    check = "bce_planted" if planted else "bce_plain"
    T = _RigidTerms(check, "lossk")
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    rows = []
    for (H, W) in LOSSK_SHAPES:
        mask = torch.sigmoid(torch.randn(B, C, H, W, generator=_lossk_gen("bce", H, W)))
        n = mask.numel()
        where = [(k * n) // len(BCE_PLANTED) for k in range(len(BCE_PLANTED))] if planted else []
        for i, v in zip(where, BCE_PLANTED):
            mask.view(-1)[i] = v
        if planted:
            assert float(mask.view(-1)[where[2]]) > 0 and float(mask.view(-1)[where[6]]) < 1        # (1e-45 and 1 - 2^-24 are fp32 values)
        r32, r64 = _bce_ones_ref(mask, F32), _bce_ones_ref(mask, F64)
        assert float(r64["terms"].min()) >= 0
        rows.append(dict(H=H, W=W, n=n, mask=mask.to(dev), where=where, r32=r32, r64=r64))

    def gmask_terms(form, d, gm):
        rest = torch.ones(d["n"], dtype=torch.bool)
        for i, v in zip(d["where"], BCE_PLANTED):
            rest[i] = False
            one = torch.zeros(d["n"], dtype=torch.bool)
            one[i] = True
            T.term("gmask_%s_planted_%.3g %dx%d" % (form, v, d["H"], d["W"]), gm, d["r32"]["g"], d["r64"]["g"], keep=one.view(gm.shape))
        T.term("gmask_%s_ordinary %dx%d" % (form, d["H"], d["W"]), gm, d["r32"]["g"], d["r64"]["g"], keep=rest.view(gm.shape))

    for d in rows:
        tag = "%dx%d" % (d["H"], d["W"])
        nbl = (d["n"] + 255) // 256
        part, loss, gm = nan(nbl + 1), torch.zeros(1, device=dev), nan(B, C, d["H"], d["W"])
        E.call("cc_bce_ones_fwd_bwd", d["mask"], gm, part, loss, LOSSK_GSCALE, d["n"], STREAM)
        T.term("loss_single " + tag, loss, d["r32"]["loss"].reshape(1), d["r64"]["loss"].reshape(1), floor=(LOSSK_K["bce_ones"] + _k_reduce(nbl)) * 2.0 ** -24)
        flat = lambda t: _piece_sums(t.reshape(1, 1, 1, -1)).reshape(-1)
        T.term("partials_single " + tag, _guarded("partials " + tag, part), flat(d["r32"]["terms"]), flat(d["r64"]["terms"]), floor=LOSSK_K["bce_ones"] * 2.0 ** -24)
        gmask_terms("single", d, gm)
    offs = _offsets([B * C * ((d["H"] * d["W"] + 255) // 256) for d in rows])
    part, loss = nan(offs[-1] + 1), torch.zeros(1, device=dev)
    gm = [nan(B, C, d["H"], d["W"]) for d in rows]
    _lossk_jobs("cc_bce_ones_fwd_bwd_jobs", [([d["mask"], gm[i], LF._off(part, offs[i])], d["H"], d["W"]) for i, d in enumerate(rows)],
                B * C, part, loss, LOSSK_GSCALE, STREAM)
    _guarded("jobs partials", part)
    T.term("loss_jobs", loss, sum(d["r32"]["loss"] for d in rows).reshape(1), sum(d["r64"]["loss"] for d in rows).reshape(1),
           floor=(LOSSK_K["bce_ones"] + _k_reduce(offs[-1])) * 2.0 ** -24)
    for i, d in enumerate(rows):
        T.term("partials_jobs %dx%d" % (d["H"], d["W"]), part[offs[i]:offs[i + 1]].view(B * C, -1), _piece_sums(d["r32"]["terms"]),
               _piece_sums(d["r64"]["terms"]), floor=LOSSK_K["bce_ones"] * 2.0 ** -24)
        gmask_terms("jobs", d, gm[i])
    T.done()


# ------------------------------------------------------------------ consensus BCE
CONSENSUS_ARGS = tuple(tuple(float(np.float32(v)) for v in a) for a in ((0.5, 0.5), (0.01, 0.2), (0.01, 0.9)))      # thresh, wbce
CONSENSUS_PLANTED = (0.0, 1.0, 1e-9, 1.0 - 2.0 ** -24)


def _consensus_inputs(H, W, thresh):
    """exp_mask = sigmoid(3 randn) with CONSENSUS_PLANTED (each twice), census values U(0, 2 thresh) with some planted exactly at
    float32(thresh) where the other channel is 0 and the target 0 (the pixel's class hangs on the strict <), targets of mean 0.3
    (bwd) and 0.7 (fwd)"""
    B, HW = LOSSK_B, H * W
    g = _lossk_gen("consensus", H, W)
    e = torch.sigmoid(3 * torch.randn(B, 4, H, W, generator=g))
    n = e.numel()
    where = [((2 * k + 1) * n) // (4 * len(CONSENSUS_PLANTED)) for k in range(2 * len(CONSENSUS_PLANTED))]
    for k, i in enumerate(where):
        e.view(-1)[i] = CONSENSUS_PLANTED[k // 2]
    cb, cf = (torch.rand(B, 2, H, W, generator=g) * (2 * thresh) for _ in range(2))
    tb, tf = (torch.rand(B, 1, H, W, generator=g) < 0.3).float(), (torch.rand(B, 1, H, W, generator=g) < 0.7).float()
    below = float(((cb < thresh).double().mean() + (cf < thresh).double().mean()) / 2)
    ties = 0
    for (c, t, b, p) in ((cb, tb, 0, 0), (cf, tf, B - 1, HW - 1)) + (((cb, tb, B - 1, HW // 2), (cf, tf, 0, HW // 2 + 1)) if HW > 16 else ()):
        y, x = p // W, p % W
        c[b, 0, y, x], c[b, 1, y, x], t[b, 0, y, x] = thresh, 0.0, 0.0
        ties += 1
    assert float((cb == thresh).sum() + (cf == thresh).sum()) == ties
    return dict(H=H, W=W, e=e, where=where, cb=cb, cf=cf, tb=tb, tf=tf, below=below)


def _consensus_ref(d, thresh, wbce, dt):
    """L.consensus_depth_flow_mask of one level in dtype dt -> loss, d loss / d exp_mask * LOSSK_GSCALE, the per-pixel terms (summed
    over the four channels), the target"""
    e = _leaf_as(d["e"], dt)
    cb, cf, tb, tf = (d[k].to(dt) for k in ("cb", "cf", "tb", "tf"))
    loss = L.consensus_depth_flow_mask([e], [cb], [cf], [tb], [tf], thresh, wbce)
    g = torch.autograd.grad(loss, e)[0] * LOSSK_GSCALE
    with torch.no_grad():
        b = L.logical_or((cb < thresh).type_as(e).prod(dim=1, keepdim=True), tb)
        f = L.logical_or((cf < thresh).type_as(e).prod(dim=1, keepdim=True), tf)
        t = torch.cat((b, b, f, f), dim=1)
        terms = -((1 - wbce) * (t * torch.log(e + L.EPS)) + wbce * ((1 - t) * torch.log(1 - e + L.EPS))) / e.numel()
    return dict(loss=loss.detach(), g=g, terms=terms.sum(1), terms4=terms, t=t)


def check_consensus_bce_float64(dev, args=CONSENSUS_ARGS):
    """cc_consensus_bce_fwd_bwd and cc_consensus_bce_fwd_bwd_jobs at LOSSK_SHAPES against L.consensus_depth_flow_mask in fp32 and
    float64 for (thresh, wbce) in CONSENSUS_ARGS (wbce != 1 - wbce is the point): loss, partials, gmask under gscale = 0.7; the planted
    exp_mask elements one by one, the ordinary ones as another term.  census and thresh are fp32 values on all sides, so `<` is the
    same decision in every precision, also at the planted equalities; 25-75 % of the census values lie below thresh and both target
    classes are present (asserted).  The terms are non-negative but for log(1 + 1e-8) where exp_mask is exactly 0 or 1: at least
    -1e-8 / n each (asserted), nothing against a loss of order 1."""
    from cc_amd._lib import engine, STREAM
    E = engine()
    B = LOSSK_B
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    T = _RigidTerms("consensus_bce", "lossk")
    for thresh, wbce in args:
        rows = []
        for (H, W) in LOSSK_SHAPES:
            d = _consensus_inputs(H, W, thresh)
            d["r32"], d["r64"] = _consensus_ref(d, thresh, wbce, F32), _consensus_ref(d, thresh, wbce, F64)
            assert float(d["r64"]["terms4"].min()) >= -1.0001e-8 / d["e"].numel(), (H, W, float(d["r64"]["terms4"].min()))
            assert torch.equal(d["r32"]["t"].double(), d["r64"]["t"])
            ones = float(d["r64"]["t"].mean())
            print("consensus_bce %dx%d thresh=%.3g: %.3f of the census values below thresh, target share %.3f" % (H, W, thresh, d["below"], ones))
            assert 0.25 <= d["below"] <= 0.75 and 0.2 <= ones <= 0.8, (H, W, d["below"], ones)
            d["dev"] = [d[k].to(dev) for k in ("e", "cb", "cf", "tb", "tf")]
            rows.append(d)

        def gmask_terms(form, d, gm):
            tag = "%dx%d thresh=%.3g wbce=%.3g" % (d["H"], d["W"], thresh, wbce)
            n = d["e"].numel()
            rest = torch.ones(n, dtype=torch.bool)
            for k, i in enumerate(d["where"]):
                rest[i] = False
                one = torch.zeros(n, dtype=torch.bool)
                one[i] = True
                T.term("gmask_%s_planted_%.3g_%d %s" % (form, CONSENSUS_PLANTED[k // 2], k % 2, tag), gm, d["r32"]["g"], d["r64"]["g"], keep=one.view(gm.shape))
            T.term("gmask_%s_ordinary %s" % (form, tag), gm, d["r32"]["g"], d["r64"]["g"], keep=rest.view(gm.shape))

        kp = LOSSK_K["consensus_bce"]
        for d in rows:
            tag = "%dx%d thresh=%.3g wbce=%.3g" % (d["H"], d["W"], thresh, wbce)
            nb = (d["H"] * d["W"] + 255) // 256
            part, loss, gm = nan(B * nb + 1), torch.zeros(1, device=dev), nan(B, 4, d["H"], d["W"])
            E.call("cc_consensus_bce_fwd_bwd", *d["dev"], gm, part, loss, thresh, wbce, LOSSK_GSCALE, B, d["H"], d["W"], STREAM)
            T.term("loss_single " + tag, loss, d["r32"]["loss"].reshape(1), d["r64"]["loss"].reshape(1), floor=(kp + _k_reduce(B * nb)) * 2.0 ** -24)
            T.term("partials_single " + tag, _guarded("partials " + tag, part).view(B, nb), _piece_sums(d["r32"]["terms"]), _piece_sums(d["r64"]["terms"]),
                   floor=kp * 2.0 ** -24)
            gmask_terms("single", d, gm)
        offs = _offsets([B * ((d["H"] * d["W"] + 255) // 256) for d in rows])
        part, loss = nan(offs[-1] + 1), torch.zeros(1, device=dev)
        gm = [nan(B, 4, d["H"], d["W"]) for d in rows]
        _lossk_jobs("cc_consensus_bce_fwd_bwd_jobs", [(d["dev"] + [gm[i], LF._off(part, offs[i])], d["H"], d["W"]) for i, d in enumerate(rows)],
                    B, part, loss, thresh, wbce, LOSSK_GSCALE, STREAM)
        _guarded("jobs partials", part)
        tag = "thresh=%.3g wbce=%.3g" % (thresh, wbce)
        T.term("loss_jobs " + tag, loss, sum(d["r32"]["loss"] for d in rows).reshape(1), sum(d["r64"]["loss"] for d in rows).reshape(1),
               floor=(kp + _k_reduce(offs[-1])) * 2.0 ** -24)
        for i, d in enumerate(rows):
            T.term("partials_jobs %dx%d %s" % (d["H"], d["W"], tag), part[offs[i]:offs[i + 1]].view(B, -1), _piece_sums(d["r32"]["terms"]),
                   _piece_sums(d["r64"]["terms"]), floor=kp * 2.0 ** -24)
            gmask_terms("jobs", d, gm[i])
    T.done()


# ------------------------------------------------------------------ decisions: occlusion masks, consensus target
def _pinned_decision(tag, outs, dec32, dec64, lhs, rhs):
    """outs: {form: device result}.  Every result (and the fp32 oracle's) equals the float64 decision dec64 wherever float64's margin
    |lhs - rhs| / max(|lhs|, |rhs|) exceeds LOSSK_DELTA; at most RIGID_MAX_EXCLUDED inside it, 20-80 % ones."""
    margin = (lhs - rhs).abs() / torch.maximum(lhs.abs(), rhs.abs()).clamp_min(1e-300)
    keep = (margin > LOSSK_DELTA).reshape(dec64.shape) if margin.shape != dec64.shape else margin > LOSSK_DELTA
    excl, ones = float((~keep).double().mean()), float(dec64.mean())
    _note("lossk:decisions:excluded_share", excl)
    print("%-64s excluded %.4f, share of ones %.3f" % (tag, excl, ones))
    assert excl <= RIGID_MAX_EXCLUDED and 0.2 <= ones <= 0.8, (tag, excl, ones)
    assert torch.equal(dec32.double()[keep], dec64[keep]), (tag, "the fp32 oracle")
    for form, o in outs.items():
        o = o.detach().cpu().double()
        assert o.shape == dec64.shape and not bool(torch.isnan(o).any()), (tag, form)
        assert torch.equal(o[keep], dec64[keep]), (tag, form, "%d decisions differ from float64's" % int((o[keep] != dec64[keep]).sum()))


def _noocc_ref(bw, fw, dt):
    """1 - L.occlusion_masks in dtype dt [B,1,H,W], and the two sides of its comparison"""
    bw, fw = bw.to(dt), fw.to(dt)
    occ_bw, occ_fw = L.occlusion_masks(bw, fw)
    assert torch.equal(occ_bw, occ_fw)
    return (1 - occ_bw).unsqueeze(1), (fw + bw).sum(dim=1, keepdim=True), (0.08 * (fw.pow(2).sum(dim=1, keepdim=True) + bw.pow(2).sum(dim=1, keepdim=True)) + 1.0)


def check_decisions_float64(dev):
    """cc_flow_noocc and cc_flow_noocc_jobs, cc_rigid_noocc, cc_consensus_target and cc_consensus_target_jobs (wrig = 0.7) at
    LOSSK_SHAPES against L.occlusion_masks and the comparison of L.consensus_exp_masks in float64 (_pinned_decision).  Flows 1.5 randn
    + 0.5: about half of the pixels are occluded."""
    from cc_amd._lib import engine, STREAM
    E = engine()
    B = LOSSK_B
    wrig = float(np.float32(0.7))
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    rows = []
    for (H, W) in LOSSK_SHAPES:
        g = _lossk_gen("decisions", H, W)
        d = dict(H=H, W=W, flows=torch.randn(4, B, 2, H, W, generator=g) * 1.5 + 0.5,
                 err_cf=torch.rand(B, 1, H, W, generator=g), err_cb=torch.rand(B, 1, H, W, generator=g), err_ff=torch.rand(B, 1, H, W, generator=g) * 0.5,
                 v_cf=(torch.rand(B, 1, H, W, generator=g) < 0.5).float(), v_cb=(torch.rand(B, 1, H, W, generator=g) < 0.5).float())
        d["dev"] = {k: v.to(dev) for k, v in d.items() if torch.is_tensor(v)}
        d["out"] = dict(noocc_jobs=nan(B * H * W + 1), target_jobs=nan(B * H * W + 1))
        rows.append(d)
    _lossk_jobs("cc_flow_noocc_jobs", [([d["dev"]["flows"][0], d["dev"]["flows"][1], d["out"]["noocc_jobs"]], d["H"], d["W"]) for d in rows], B, STREAM)
    _lossk_jobs("cc_consensus_target_jobs", [([d["dev"][k] for k in ("err_cf", "err_cb", "err_ff", "v_cf", "v_cb")] + [d["out"]["target_jobs"]], d["H"], d["W"])
                                             for d in rows], B, wrig, STREAM)
    for d in rows:
        H, W, v = d["H"], d["W"], d["dev"]
        tag = "%dx%d" % (H, W)
        # occlusion_masks(flow_bw, flow_fw) of flows 0 and 1
        single = nan(B * H * W + 1)
        E.call("cc_flow_noocc", v["flows"][0], v["flows"][1], single, B, H, W, STREAM)
        outs = {k: _guarded(k + " " + tag, t).view(B, 1, H, W) for k, t in (("single", single), ("jobs", d["out"]["noocc_jobs"]))}
        r32, r64 = _noocc_ref(d["flows"][0], d["flows"][1], F32), _noocc_ref(d["flows"][0], d["flows"][1], F64)
        _pinned_decision("flow_noocc " + tag, outs, r32[0], r64[0], r64[1], r64[2])
        # depth_occlusion_masks' pairing of four flows: (m03, m12, m12, m03)
        out4 = nan(B * 4 * H * W + 1)
        E.call("cc_rigid_noocc", v["flows"], out4, B, H, W, STREAM)
        ref = {}
        for dt in (F32, F64):
            m12, m03 = _noocc_ref(d["flows"][1], d["flows"][2], dt), _noocc_ref(d["flows"][0], d["flows"][3], dt)
            ref[dt] = [torch.cat([m[k] for m in (m03, m12, m12, m03)], 1) for k in range(3)]
        _pinned_decision("rigid_noocc " + tag, dict(single=_guarded("rigid_noocc " + tag, out4).view(B, 4, H, W)), ref[F32][0], ref[F64][0], ref[F64][1], ref[F64][2])
        # the consensus target
        single = nan(B * H * W + 1)
        E.call("cc_consensus_target", v["err_cf"], v["err_cb"], v["err_ff"], v["v_cf"], v["v_cb"], single, wrig, B * H * W, STREAM)
        outs = {k: _guarded(k + " " + tag, t).view(B, 1, H, W) for k, t in (("single", single), ("jobs", d["out"]["target_jobs"]))}
        ref = {}
        for dt in (F32, F64):
            cam_err = torch.min(d["err_cf"].to(dt), d["err_cb"].to(dt)) * L.logical_or(d["v_cf"].to(dt), d["v_cb"].to(dt))
            lhs, rhs = wrig * cam_err, d["err_ff"].to(dt) + L.EPS
            ref[dt] = ((lhs <= rhs).to(dt), lhs, rhs)
        _pinned_decision("consensus_target " + tag, outs, ref[F32][0], ref[F64][0], ref[F64][1], ref[F64][2])


# ------------------------------------------------------------------ k_reduce_add
REDUCE_NS = (1, 255, 256, 2048, 2049, 5000, 20000)         # one work-item's eight loads cover 2048 partials; 20000 > 8 * 2048


def check_reduce_add_float64(dev):
    """cc_reduce_add: accum (0.5 before the call) += coef * sum(partials[0..n)) with coef = float32(0.3), non-negative partials,
    against float64 under the floor of the sums (k = _k_reduce(n) + 1 for the product); the NaN behind partials[n - 1] is not read."""
    from cc_amd._lib import engine, STREAM
    E = engine()
    T = _RigidTerms("reduce_add", "lossk")
    coef, acc0 = float(np.float32(0.3)), 0.5
    for n in REDUCE_NS:
        part = torch.full((n + 300,), float("nan"))
        part[:n] = torch.rand(n, generator=torch.Generator().manual_seed(n))
        acc = torch.full((1,), acc0, device=dev)
        E.call("cc_reduce_add", part.to(dev), n, coef, acc, STREAM)
        assert bool(torch.isfinite(acc).all()), (n, "read behind partials[n - 1]")
        r32 = torch.full((1,), acc0) + torch.tensor(coef) * part[:n].sum()
        r64 = acc0 + coef * part[:n].double().sum()
        T.term("accum n=%d" % n, acc, r32, r64.reshape(1), floor=(_k_reduce(n) + 1) * 2.0 ** -24)
    T.done()


# ------------------------------------------------------------------ element-wise jobs
def check_elementwise_jobs_float64(dev):
    """cc_elementwise_jobs, two rows (8x26, 20x53) per launch: ops 0 (1 / a), 1 (-g y^2) and 5 (ImageNet normalisation) against
    float64 under the per-pixel bar; ops 2 (|a - b|), 3 (1 - m[:, c0:c0 + nc]) and 4 (its backward: exactly 0 outside the slice, over
    a sentinel-filled output; c0 = 1, nc = 2, MC = 4) exactly."""
    from cc_amd._lib import STREAM
    B = LOSSK_B
    T = _RigidTerms("elementwise", "lossk")
    hw = LOSSK_SHAPES[:2]
    g = torch.Generator().manual_seed(17)

    def run(op, planes, ins, out_planes, c0=0, nc=0, MC=0, fill=float("nan")):
        """ins: per input a list with one tensor per row -> the rows' outputs [out_planes, H, W]"""
        outs = [torch.full((out_planes * H * W + 1,), fill, device=dev) for H, W in hw]
        _lossk_jobs("cc_elementwise_jobs", [([t[i].to(dev) for t in ins] + [outs[i]], H, W) for i, (H, W) in enumerate(hw)], planes, op, c0, nc, MC, STREAM)
        res = []
        for o, (H, W) in zip(outs, hw):
            assert float(o[-1]) != float(o[-1]) or float(o[-1]) == fill, "a write behind the documented extent"
            assert not bool(torch.isnan(o[:-1]).any()) and (fill != fill or not bool((o[:-1] == fill).any())), "an element was not written"
            res.append(o[:-1].view(out_planes, H, W).cpu())
        return res

    P = B * 3
    a = [torch.rand(P, H, W, generator=g) + 0.25 for H, W in hw]
    gr = [torch.randn(P, H, W, generator=g) for H, W in hw]
    y = run(0, P, [a], P)
    ga = run(1, P, [gr, y], P)
    im = [torch.rand(P, H, W, generator=g) * 2 - 1 for H, W in hw]
    nrm = run(5, P, [im], P)
    for i, (H, W) in enumerate(hw):
        tag = "%dx%d" % (H, W)
        T.term("op0 " + tag, y[i], 1.0 / a[i], 1.0 / a[i].double())
        T.term("op1 " + tag, ga[i], -gr[i] * (y[i] * y[i]), -gr[i].double() * (y[i].double() * y[i].double()))
        stat = lambda dt: [torch.tensor(s, dtype=dt).repeat(B).view(P, 1, 1) for s in ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))]
        ref = {dt: ((im[i].to(dt) * 0.5 + 0.5) - stat(dt)[0]) / stat(dt)[1] for dt in (F32, F64)}
        T.term("op5 " + tag, nrm[i], ref[F32], ref[F64])
    b_ = [torch.rand(P, H, W, generator=g) for H, W in hw]
    for i, o in enumerate(run(2, P, [a, b_], P)):
        assert torch.equal(o, (a[i] - b_[i]).abs()), ("op 2", i)
    c0, nc, MC = 1, 2, 4
    m = [torch.rand(B, MC, H, W, generator=g) for H, W in hw]
    for i, o in enumerate(run(3, B * nc, [m], B * nc, c0, nc, MC)):
        assert torch.equal(o.view(B, nc, *hw[i]), 1.0 - m[i][:, c0:c0 + nc]), ("op 3", i)
    gs = [torch.randn(B, nc, H, W, generator=g) for H, W in hw]
    for i, o in enumerate(run(4, B * MC, [gs], B * MC, c0, nc, MC, fill=-77.0)):
        o = o.view(B, MC, *hw[i])
        assert torch.equal(o[:, c0:c0 + nc], -gs[i]), ("op 4: the slice", i)
        assert bool((o[:, :c0] == 0).all()) and bool((o[:, c0 + nc:] == 0).all()), ("op 4: not exactly 0 outside the slice", i)
    T.done()


# ------------------------------------------------------------------ the pyramid's fallbacks
def check_pyramid_fallbacks_float64(dev):
    """cc_pyramid_build where the one-launch tile kernel does not apply: 48x80 (not a multiple of 32: one k_adaptive_pool launch per
    level) and 64x96 from a pointer 4 bytes behind a 16-byte boundary (the alignment fallback; the aligned call beside it).  Every
    level is torch.equal to cc_adaptive_avg_pool of that level and held to F.adaptive_avg_pool2d in float64 under the per-pixel bar."""
    import torch.nn.functional as F
    from cc_amd._lib import engine, STREAM
    E = engine()
    T = _RigidTerms("pyramid", "lossk")
    B, nlevels = LOSSK_B, 6
    for (H, W, off) in ((48, 80, 0), (64, 96, 1), (64, 96, 0)):
        x = syn.frames(B, H, W, seed=11, n_frames=1)[0]
        xd = _at_offset(x.to(dev), off)
        sizes = [(H >> l, W >> l) for l in range(1, nlevels)]
        packed = torch.full((sum(B * 3 * h * w for h, w in sizes) + 1,), float("nan"), device=dev)
        E.call("cc_pyramid_build", xd, packed, nlevels, B * 3, H, W, STREAM)
        body, o = _guarded("pyramid %dx%d" % (H, W), packed), 0
        for (h, w) in sizes:
            tag = "%dx%d+%d -> %dx%d" % (H, W, off, h, w)
            lv = body[o:o + B * 3 * h * w].view(B, 3, h, w)
            o += B * 3 * h * w
            pool = torch.full((B, 3, h, w), float("nan"), device=dev)
            E.call("cc_adaptive_avg_pool", xd, pool, B * 3, H, W, h, w, STREAM)
            assert torch.equal(lv, pool), (tag, "differs from cc_adaptive_avg_pool")
            T.term("level " + tag, lv, F.adaptive_avg_pool2d(x, (h, w)), F.adaptive_avg_pool2d(x.double(), (h, w)))
    T.done()
