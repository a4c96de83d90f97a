"""FlowNetC6 in the trainer's step, shared by tests/test_flownetc_step.py (x86 emulation build) and tests/test_flownetc_step_gpu.py:

  1. the plane-GEMM cost-volume kernels (cc_corr_plane_{fwd,bwd}, csrc/corr_plane.hip) against float64 and against the gather
     kernels (cc_corr_patch_*) they replace where their predicate holds;
  2. FlowNetC6Ref, a restatement of the network from torch.nn.functional and oracle.corr, pinned to tests/golden/altnets.npz the way
     tests/test_alt_nets.py pins the engine's module -- the reference of 3 and 4;
  3. FlowNetC6.forward_pair against two calls;
  4. CCTrainer with [DispResNet6, PoseNetB6, MaskNet6, FlowNetC6] against oracle.step with the restatement in its flow slot;
  5. Back2Future's step with config.debug.corr_patch_gather on and off: same engine calls, same results."""
import functools
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from cc_amd import config, models, ops, synthetic as syn, trainer as T
from cc_amd._lib import engine, STREAM
from oracle import corr as OC, step as S

P, D, ND = 21, 2, 441
KERNEL_CASES = [(1, 3, 2, 2),          # planes of one pixel
                (2, 5, 8, 16),         # the 64 x 128 frame's map: every window covers the plane
                (1, 6, 44, 48),        # every displacement lands inside somewhere; planes wider than one tile in both directions
                (2, 70, 6, 36),        # C not a multiple of any K step
                (1, 256, 8, 16),       # the network's C
                (2, 64, 32, 104)]      # the training map
REFUSED_CASE = (1, 3, 6, 7)            # odd width: the predicate says no
SB, SH, SW = 2, 64, 128                # the step's batch


# ----------------------------------------------------------------------------- 1. kernels
def _inputs(case):
    B, C, H, W = case
    g = torch.Generator().manual_seed(1000 + B * 7 + C * 13 + H * 17 + W)
    return (torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g), torch.randn(B, ND, H, W, generator=g))


@functools.lru_cache(maxsize=None)
def float64_reference(case):
    """oracle.corr.correlation_volume / C and its autograd gradients in float64 on the case's fp32 inputs; computed once per
    process, never modified.  -> (out, g1, g2, in-map mask [441, H, W])"""
    B, C, H, W = case
    f1, f2, gout = _inputs(case)
    a, b = f1.double().requires_grad_(True), f2.double().requires_grad_(True)
    vol = OC.correlation_volume(a, b, P, D).reshape(B, ND, H, W) / C
    g1, g2 = torch.autograd.grad(vol, (a, b), gout.double())
    r = (P - 1) // 2
    off = (torch.arange(P) - r) * D
    yy = torch.arange(H)[None, :] + off[:, None]                        # [P, H]
    xx = torch.arange(W)[None, :] + off[:, None]                        # [P, W]
    iny, inx = (yy >= 0) & (yy < H), (xx >= 0) & (xx < W)
    inmap = (iny[:, None, :, None] & inx[None, :, None, :]).reshape(ND, H, W)
    return vol.detach(), g1, g2, inmap


def _e(x, ref):
    return float((x.detach().double().cpu() - ref).abs().max() / ref.abs().max())


class _Names:
    """the entry points ops.correlate_patch called"""

    def __enter__(self):
        self.e, self.names = engine(), []
        orig = self.e.call

        def call(name, *a):
            if name.startswith("cc_corr_"):
                self.names.append(name)
            return orig(name, *a)
        self.e.call = call
        return self

    def __exit__(self, *a):
        del self.e.call
        return False


def _through_ops(f1, f2, gout, gather):
    old = config.debug.corr_patch_gather
    config.debug.corr_patch_gather = gather
    try:
        a, b = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
        with _Names() as log:
            out = ops.correlate_patch(a, b, P, D)
            out.backward(gout)
        return (out.detach(), a.grad, b.grad), log.names
    finally:
        config.debug.corr_patch_gather = old


def check_kernels(dev, case):
    B, C, H, W = case
    r64, g1_64, g2_64, inmap = float64_reference(case)
    f1, f2, gout = [t.to(dev) for t in _inputs(case)]
    nan = float("nan")
    E = engine()

    def fwd():
        out = torch.full((B, ND, H, W), nan, device=dev)
        E.call("cc_corr_plane_fwd", f1, f2, out, B, C, H, W, P, D, STREAM)
        return out

    def bwd(want1=True, want2=True):
        g1 = torch.full((B, C, H, W), nan, device=dev) if want1 else None
        g2 = torch.full((B, C, H, W), nan, device=dev) if want2 else None
        E.call("cc_corr_plane_bwd", gout, f1, f2, g1, g2, B, C, H, W, P, D, STREAM)
        return g1, g2
    out = fwd()
    g1, g2 = bwd()
    for name, t in (("out", out), ("g1", g1), ("g2", g2)):
        assert not bool(torch.isnan(t).any()), (case, name, "not fully written")
    outside = ~inmap.to(dev)[None].expand(B, ND, H, W)
    assert bool((out[outside] == 0).all()), (case, "non-zero where the displacement leaves the map")
    # two runs of every entry: the same bits; a null gradient leaves the other one unchanged
    assert torch.equal(fwd(), out)
    g1b, g2b = bwd()
    assert torch.equal(g1b, g1) and torch.equal(g2b, g2)
    assert torch.equal(bwd(want2=False)[0], g1) and torch.equal(bwd(want1=False)[1], g2)
    # both paths through ops.correlate_patch and the debug switch, same inputs
    new, names_new = _through_ops(f1, f2, gout, gather=False)
    old, names_old = _through_ops(f1, f2, gout, gather=True)
    assert names_new == ["cc_corr_plane_fwd", "cc_corr_plane_bwd"] and names_old == ["cc_corr_patch_fwd", "cc_corr_patch_bwd"]
    assert torch.equal(new[0], out) and torch.equal(new[1], g1) and torch.equal(new[2], g2)
    for name, x_new, x_old, ref, bar in (("out", new[0], old[0], r64, 2e-6), ("g1", new[1], old[1], g1_64, 5e-6),
                                         ("g2", new[2], old[2], g2_64, 5e-6)):
        e_new, e_old = _e(x_new, ref), _e(x_old, ref)
        print("corr_plane %s %-3s e_new %.3e  e_gather %.3e" % (case, name, e_new, e_old))
        assert e_new <= 2 * e_old, (case, name, e_new, e_old)
        if e_old < bar:
            assert e_new < bar, (case, name, e_new, e_old)
        # the K order of every plane GEMM is the gather kernels' summation order: the same bits
        assert torch.equal(x_new, x_old), (case, name, float((x_new - x_old).abs().max()))


def check_fall_through(dev):
    """a shape the predicate refuses: ops.correlate_patch runs the gather kernels whatever the switch says, and the plane entries
    themselves answer CC_ERR_ARG before anything is launched"""
    B, C, H, W = REFUSED_CASE
    f1, f2, gout = [t.to(dev) for t in _inputs(REFUSED_CASE)]
    a, na = _through_ops(f1, f2, gout, gather=False)
    b, nb = _through_ops(f1, f2, gout, gather=True)
    assert na == nb == ["cc_corr_patch_fwd", "cc_corr_patch_bwd"]
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    out = torch.zeros(B, ND, H, W, device=dev)
    for args in ((B, C, H, W, P, D), (B, C, 6, 8, 9, D), (B, C, 6, 8, P, 1), (0, C, 6, 8, P, D)):
        try:
            engine().call("cc_corr_plane_fwd", f1, f2, out, *args, STREAM)
        except RuntimeError as err:
            assert "failed with code -1" in str(err)
        else:
            raise AssertionError("cc_corr_plane_fwd accepted %r" % (args,))
    assert float(out.abs().max()) == 0


# ----------------------------------------------------------------------------- 2. the restatement
class FlowNetC6Ref(nn.Module):
    """FlowNetC with a 21 x 21 / dilation-2 cost volume on the 1/8 features (models/FlowNetC6.py of the reference, batchNorm=False,
    div_flow 20, full_res): torch.nn.functional convolutions over parameters that carry the reference's state_dict keys, and
    oracle.corr for the cost volume.  forward(x1, x2) -> the six levels (what the reference returns in train mode); level 0 alone
    is its eval-mode result."""
    SLOPE, DIV = 0.1, 20

    def __init__(self):
        super().__init__()

        def conv(cin, cout, k=3, stride=1):
            return nn.Sequential(nn.Conv2d(cin, cout, k, stride, (k - 1) // 2), nn.LeakyReLU(self.SLOPE))

        def deconv(cin, cout):
            return nn.Sequential(nn.ConvTranspose2d(cin, cout, 4, 2, 1), nn.LeakyReLU(self.SLOPE))
        self.conv1, self.conv2, self.conv3 = conv(3, 64, 7, 2), conv(64, 128, 5, 2), conv(128, 256, 5, 2)
        self.conv_redir = conv(256, 32, 1, 1)
        self.conv3_1 = conv(473, 256)
        self.conv4, self.conv4_1 = conv(256, 512, stride=2), conv(512, 512)
        self.conv5, self.conv5_1 = conv(512, 512, stride=2), conv(512, 512)
        self.conv6, self.conv6_1 = conv(512, 1024, stride=2), conv(1024, 1024)
        self.deconv5, self.deconv4, self.deconv3 = deconv(1024, 512), deconv(1026, 256), deconv(770, 128)
        self.deconv2, self.deconv1 = deconv(386, 64), deconv(194, 32)
        for lvl, cin in zip(range(6, 0, -1), (1024, 1026, 770, 386, 194, 98)):
            setattr(self, "predict_flow%d" % lvl, nn.Conv2d(cin, 2, 3, 1, 1))
        for a, b in ((6, 5), (5, 4), (4, 3), (3, 2), (2, 1)):
            setattr(self, "upsampled_flow%d_to_%d" % (a, b), nn.ConvTranspose2d(2, 2, 4, 2, 1))

    def _c(self, seq, x):
        m = seq[0]
        return F.leaky_relu(F.conv2d(x, m.weight, m.bias, m.stride, m.padding), self.SLOPE)

    def _d(self, seq, x):
        m = seq[0]
        return F.leaky_relu(F.conv_transpose2d(x, m.weight, m.bias, 2, 1), self.SLOPE)

    def forward(self, x1, x2):
        c1a = self._c(self.conv1, x1)
        c2a = self._c(self.conv2, c1a)
        c3a = self._c(self.conv3, c2a)
        c3b = self._c(self.conv3, self._c(self.conv2, self._c(self.conv1, x2)))
        vol = OC.correlation_volume(c3a, c3b, P, D)
        b, ph, pw, h, w = vol.shape
        corr = F.leaky_relu(vol.reshape(b, ph * pw, h, w) / c3a.size(1), self.SLOPE)
        c31 = self._c(self.conv3_1, torch.cat((self._c(self.conv_redir, c3a), corr), 1))
        c4 = self._c(self.conv4_1, self._c(self.conv4, c31))
        c5 = self._c(self.conv5_1, self._c(self.conv5, c4))
        c6 = self._c(self.conv6_1, self._c(self.conv6, c5))
        flows = {6: self._p(6, c6)}
        feat = c6
        for lvl, skip in ((5, c5), (4, c4), (3, c31), (2, c2a), (1, c1a)):
            dec = self._d(getattr(self, "deconv%d" % lvl), feat)
            m = getattr(self, "upsampled_flow%d_to_%d" % (lvl + 1, lvl))
            up = F.conv_transpose2d(flows[lvl + 1], m.weight, m.bias, 2, 1)
            feat = torch.cat((skip, dec, up), 1)
            flows[lvl] = self._p(lvl, feat)
        return tuple(self.DIV * F.interpolate(flows[l], scale_factor=2, mode="bilinear", align_corners=False) for l in range(1, 7))

    def _p(self, lvl, x):
        m = getattr(self, "predict_flow%d" % lvl)
        return F.conv2d(x, m.weight, m.bias, 1, 1)


def seeded_ref(dtype=torch.float32):
    net = FlowNetC6Ref()
    net.load_state_dict(syn.seeded_state_dict(models.FlowNetC6(nlevels=6), 0))       # the engine module's keys, in its order
    return net.to(dtype).train()


def _rel(a, b):
    a, b = a.detach().cpu().reshape(-1), b.detach().cpu().reshape(-1)
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def check_restatement_against_golden(golden_dir):
    """tests/test_alt_nets.py::_check for the restatement: the reference module's train-mode outputs on the seeded sample within
    1e-4, its parameter-gradient norm within 2e-3"""
    from oracle.make_golden import AB, AH, AW, alt_net_args
    gold = np.load(os.path.join(golden_dir, "altnets.npz"))
    tgt, refs, _, _ = syn.sample(AB, AH, AW, seed=1)
    net = seeded_ref()
    assert list(net.state_dict().keys()) == list(models.FlowNetC6(nlevels=6).state_dict().keys())
    outs = list(net(*alt_net_args("FlowNetC6", tgt, refs)))
    assert len(outs) == 6
    for i, o in enumerate(outs):
        k = "FlowNetC6.%d" % i
        flat = o.detach().reshape(-1)
        if k in gold:
            ref = torch.from_numpy(gold[k]).reshape(-1)
            assert float((flat - ref).abs().max() / (ref.abs().max() + 1e-30)) < 1e-4, k
        else:
            st = gold[k + ".stats"]
            assert abs(float(flat.double().sum()) - st[0]) <= 1e-4 * st[1], k
            ref = torch.from_numpy(gold[k + ".sample"])
            got = flat[:: max(1, flat.numel() // 2048)]
            assert float((got - ref).abs().max() / (ref.abs().max() + 1e-30)) < 1e-4, k
    sum((o * o).mean() for o in outs).backward()
    gn = sum(float(p.grad.double().pow(2).sum()) for p in net.parameters()) ** 0.5
    want = float(gold["FlowNetC6.gradnorm"])
    assert abs(gn - want) <= 2e-3 * want, (gn, want)


# ----------------------------------------------------------------------------- 3. forward_pair
def _gradnorm(net, outs):
    net.zero_grad()
    sum((o * o).mean() for o in outs).backward()
    return sum(float(p.grad.double().pow(2).sum()) for p in net.parameters() if p.grad is not None) ** 0.5


@functools.lru_cache(maxsize=None)
def ref_two_calls():
    """the restatement's two calls (flow_fwd: refs[2], flow_bwd: refs[1]) on the step's batch and the gradient norm of the fixed
    scalar sum(mean(o^2)) over the twelve outputs; float32, on the host, computed once"""
    tgt, refs, _, _ = syn.sample(SB, SH, SW, seed=1)
    net = seeded_ref()
    fwd, bwd = net(tgt, refs[2]), net(tgt, refs[1])
    gn = _gradnorm(net, list(fwd) + list(bwd))
    return [o.detach() for o in fwd], [o.detach() for o in bwd], gn


def check_forward_pair(dev):
    tgt, refs, _, _ = syn.sample(SB, SH, SW, seed=1)
    t, r_fwd, r_bwd = tgt.to(dev), refs[2].to(dev), refs[1].to(dev)
    net = models.FlowNetC6(nlevels=6)
    net.load_state_dict(syn.seeded_state_dict(net, 0))
    net.to(dev).train()
    pair = net.forward_pair(t, [r_fwd, r_bwd])
    assert isinstance(pair, tuple) and len(pair) == 2 and all(isinstance(p, tuple) and len(p) == 6 for p in pair)
    gn_pair = _gradnorm(net, list(pair[0]) + list(pair[1]))
    two = (net(t, r_fwd), net(t, r_bwd))
    gn_two = _gradnorm(net, list(two[0]) + list(two[1]))
    want_fwd, want_bwd, gn_ref = ref_two_calls()
    for got, own, want in ((pair[0], two[0], want_fwd), (pair[1], two[1], want_bwd)):
        for lvl in range(6):
            assert got[lvl].shape == own[lvl].shape == want[lvl].shape
            assert _rel(got[lvl], own[lvl]) < 1e-4 and _rel(got[lvl], want[lvl]) < 1e-4, (lvl, _rel(got[lvl], own[lvl]), _rel(got[lvl], want[lvl]))
    assert abs(gn_pair - gn_two) <= 2e-3 * gn_two and abs(gn_pair - gn_ref) <= 2e-3 * gn_ref, (gn_pair, gn_two, gn_ref)
    net.eval()
    with torch.no_grad():
        ef, eb = net.forward_pair(t, [r_fwd, r_bwd])
        of, ob = net(t, r_fwd), net(t, r_bwd)
    assert torch.is_tensor(ef) and torch.is_tensor(eb) and ef.shape == of.shape == (SB, 2, SH, SW)
    assert _rel(ef, of) < 1e-4 and _rel(eb, ob) < 1e-4 and _rel(ef, want_fwd[0]) < 1e-4 and _rel(eb, want_bwd[0]) < 1e-4


# ----------------------------------------------------------------------------- 4. the step
class FlowSlot(nn.Module):
    """the oracle step's flow slot over the restatement: (tgt, refs[1:3]) -> (flow_fwd levels, flow_bwd levels, None), the
    two calls of train.py:465-466 (flow_fwd from refs[2], flow_bwd from refs[1])"""

    def __init__(self, net, eval_levels=False):
        super().__init__()
        self.net, self.eval_levels = net, eval_levels

    def forward(self, tgt, refs):
        fwd, bwd = self.net(tgt, refs[1]), self.net(tgt, refs[0])
        if self.eval_levels:
            return [fwd[0]], [bwd[0]], None
        return list(fwd), list(bwd), None


def seeded_nets(dev):
    nets = T.build_nets(dev, init=False, flownet="FlowNetC6")
    assert isinstance(nets[3], models.FlowNetC6)
    for n in nets:
        n.load_state_dict(syn.seeded_state_dict(n, 0))
    return nets


def oracle_nets(dtype=torch.float32):
    onets = S.build_nets("oracle")
    for n in onets[:3]:
        n.load_state_dict(syn.seeded_state_dict(n, 0))
    onets[3] = FlowSlot(seeded_ref())
    for n in onets:
        n.to(dtype).train()
    return onets


@functools.lru_cache(maxsize=None)
def oracle_step():
    """oracle.step.cc_step on the seeded 2 x 64 x 128 batch with the restatement in the flow slot, once per process:
    -> (six losses, per-network gradient norms, parameters after the Adam step in bucket order)"""
    batch = syn.sample(SB, SH, SW, seed=1)
    onets = oracle_nets()
    ocfg = S.StepConfig()
    losses = S.cc_step(onets, S.make_optimizer(onets, ocfg), batch, ocfg)
    norms = {name: sum(float(p.grad.double().pow(2).sum()) for p in n.parameters()) ** 0.5 for name, n in zip(T.NET_NAMES, onets)}
    params = torch.cat([p.detach().reshape(-1) for n in onets for p in n.parameters()])
    return losses, norms, params


def step_batch(dev):
    b = syn.sample(SB, SH, SW, seed=1)
    return (b[0].to(dev), [r.to(dev) for r in b[1]], b[2].to(dev), b[3].to(dev))


def check_step_against_oracle(dev):
    """one eager CCTrainer step with FlowNetC6 in the flow slot: the six losses within 1e-4 (tests/test_step_emu.py,
    tests/test_headline_gpu.py), the per-network gradient norms within 1e-3 (test_headline_gpu), the parameters after the Adam step as
    test_step_emu compares them (first step: |update| = lr wherever the gradient is not ~0, so fewer than 1e-3 of the elements may
    differ by more than 1e-6 and none by more than 2 lr)"""
    want, want_norms, want_params = oracle_step()
    tr = T.CCTrainer(seeded_nets(dev), T.StepConfig(), use_graph=False)
    assert tr.pipeline == "per_network"
    got = {k: float(v) for k, v in tr.step(step_batch(dev)).items()}
    for k, v in want.items():
        print("FlowNetC6 step %-7s engine %.8f  oracle %.8f  rel %.2e" % (k, got[k], v, abs(got[k] - v) / abs(v)))
    for name, v in tr.grad_norms().items():
        print("FlowNetC6 step gradnorm %-5s engine %.8e  oracle %.8e  rel %.2e" % (name, float(v), want_norms[name],
                                                                                  abs(float(v) - want_norms[name]) / want_norms[name]))
    for k, v in want.items():
        assert abs(got[k] - v) <= 1e-4 * abs(v), (k, got[k], v)
    for name, v in tr.grad_norms().items():
        assert abs(float(v) - want_norms[name]) <= 1e-3 * want_norms[name], (name, float(v), want_norms[name])
    d = (tr.opt.gather(tr.opt.flat_p).cpu() - want_params).abs()
    assert float((d > 1e-6).float().mean()) < 1e-3 and float(d.max()) <= 2.001e-4, (float((d > 1e-6).float().mean()), float(d.max()))
    tr.check_finite()
    return tr


def check_legacy_forms_refused(dev):
    nets = seeded_nets(dev)
    for form in ("post", "staged"):
        try:
            T.CCTrainer(nets, T.StepConfig(), use_graph=False, pipeline=form)
        except ValueError as err:
            assert "two-frame flow network" in str(err) and "per_network" in str(err)
        else:
            raise AssertionError("pipeline=%r accepted FlowNetC6" % form)


def check_validation_pass(dev, tmp):
    """validate.validate_without_gt_from_store with the four networks in eval mode against the oracle's forward-only losses over
    one-level lists (tests/test_train_gpu.py::test_unsupervised_pass_against_oracle, its 1e-4)"""
    import train_cases as C
    from cc_amd import custom_transforms as CT, datasets as DS, validate as V
    root = C.data_tree(tmp)
    store = DS.FrameStore.build(root, train=False, sequence_length=5, device=dev, workers=2)
    assert len(store) == 2 and tuple(store.frames.shape[1:3]) == (C.LH, C.LW)
    x = CT.DeviceFrames(device=dev).store_to_tensor(store, store.samples_np.T.reshape(-1)).view(5, 2, 3, C.LH, C.LW).cpu()
    K = torch.from_numpy(store.intrinsics_np[store.sample_scene_np])
    batch = (x[0], [x[j] for j in range(1, 5)], K, torch.from_numpy(np.stack([np.linalg.inv(k) for k in K.numpy()])))
    onets = oracle_nets()
    for n in onets:
        n.eval()
    onets[3].eval_levels = True
    with torch.no_grad():
        as_levels = (lambda t: [onets[0](t)], onets[1], lambda t, r: [onets[2](t, r)], onets[3])
        want = {k: float(v) for k, v in S.cc_forward(as_levels, batch, S.StepConfig()).items() if k.startswith("loss")}
    nets = seeded_nets(dev)
    got, names = V.validate_without_gt_from_store(store, *nets, 2, T.StepConfig())
    assert names == ["loss", "loss_1", "loss_2", "loss_3", "loss_4", "loss_5"] and all(not n.training for n in nets)
    for k, g in zip(names, got):
        print("FlowNetC6 unsupervised %-7s engine %.8f  oracle %.8f  rel %.2e" % (k, g, want[k], abs(g - want[k]) / abs(want[k])))
    for k, g in zip(names, got):
        assert want[k] != 0 and abs(g - want[k]) <= 1e-4 * abs(want[k]), (k, g, want[k])


def _restore_after(tr, fn):
    """what CCTrainer.capture() does around its warm-up, for an eager trainer: fn(), then parameters, moments and counter are put
    back (a trainer's very first step finds no weight images registered and takes another split of some grouped reductions; every
    step of a captured trainer runs behind capture()'s warm-up)"""
    opt = tr.opt
    keep = [(t, t.detach().clone()) for t in (opt.flat_p, opt.exp_avg, opt.exp_avg_sq, opt.step_dev)] + \
           [(b, b.detach().clone()) for n in tr.nets for b in n.buffers()]
    fn()
    torch.cuda.synchronize()
    for t, saved in keep:
        t.copy_(saved)


def check_captured_equals_eager(dev, monkeypatch):
    """config.deterministic: three replays of the captured step == three eager steps, bit for bit (losses and parameters)"""
    monkeypatch.setattr(config, "deterministic", True)
    batch = step_batch(dev)
    eager = T.CCTrainer(seeded_nets(dev), T.StepConfig(), use_graph=False)
    _restore_after(eager, lambda: eager.step(batch))
    le = [{k: float(v) for k, v in eager.step(batch).items()} for _ in range(3)]
    pe = eager.opt.flat_p.clone()
    cap = T.CCTrainer(seeded_nets(dev), T.StepConfig(), use_graph=True)
    try:
        lc = [{k: float(v) for k, v in cap.step(batch).items()} for _ in range(3)]
        assert cap.graph is not None and cap.pipeline == "per_network" and float(cap.opt.step_dev) == 3.0
        assert all(np.isfinite(v) for l in lc for v in l.values()) and lc[0]["loss"] != lc[1]["loss"] != lc[2]["loss"]
        assert le == lc, (le, lc)
        assert torch.equal(pe, cap.opt.flat_p)
        cap.check_finite()
    finally:
        # the graph and its private pool go now, with the test, not whenever the cycle collector finds the dead trainer (which may be
        # in the middle of a later test's capture)
        torch.cuda.synchronize()
        if cap.graph is not None:
            cap.graph.reset()
        cap.graph = cap.static_batch = cap.losses = None
        cap.nan_flags = []


# ----------------------------------------------------------------------------- 5. nothing moved
def check_back2future_step_unmoved(dev):
    """Back2Future in the flow slot, config.debug.corr_patch_gather on and off: the step makes the same engine calls with the same
    arguments (tests/loss_calls.py ArgLog over the whole step) and leaves the same losses, gradients and parameters"""
    import ctypes
    from loss_calls import ArgLog

    class StepLog(ArgLog):                  # every call of the step; an address (job tables included) is "p", 0 when null
        def arg(self, name, a, v, ty, an):
            if ty is ctypes.c_void_p:
                return 0 if (v is None or (isinstance(v, int) and v == 0)) else "p"
            return v
    batch = step_batch(dev)
    res = []
    old = config.debug.corr_patch_gather
    try:
        # (the first run is thrown away: both compared steps then follow a Back2Future trainer of this process -- what a trainer
        # finds registered by its predecessor, weight images and per-stream queues, is the same for both)
        for gather in (False, False, True):
            config.debug.corr_patch_gather = gather
            nets = T.build_nets(dev, init=False)
            assert isinstance(nets[3], models.Back2Future) and not hasattr(nets[3], "forward_pair")
            for n in nets:
                n.load_state_dict(syn.seeded_state_dict(n, 0))
            tr = T.CCTrainer(nets, T.StepConfig(), use_graph=False)
            with StepLog() as log:
                losses = {k: float(v) for k, v in tr.step(batch).items()}
            res.append((log.calls, losses, tr.opt.flat_g.clone(), tr.opt.flat_p.clone()))
    finally:
        config.debug.corr_patch_gather = old
    (ca, la, ga, pa), (cb, lb, gb, pb) = res[1:]
    na, nb = [c[0] for c in ca], [c[0] for c in cb]
    first = next((k for k, (x, y) in enumerate(zip(na, nb)) if x != y), min(len(na), len(nb)))
    assert len(ca) > 100 and na == nb, (len(na), len(nb), first, na[first - 2:first + 3], nb[first - 2:first + 3])
    assert not any(c[0].startswith("cc_corr_p") for c in ca) and any(c[0] == "cc_corr9x9_fwd" for c in ca)
    assert ca == cb
    assert la == lb and torch.equal(ga, gb) and torch.equal(pa, pb)
