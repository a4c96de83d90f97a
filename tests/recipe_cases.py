"""Shared bodies of tests/test_recipe.py (x86 emulation build) and tests/test_recipe_gpu.py (MI355X): the two recipe switches of
train.py the step takes -- StepConfig.spatial_normalize (train.py:455-456) and StepConfig.no_non_rigid_mask (train.py:483-488) --
and the kernels under the first one (cc_spatial_norm_fwd_jobs / cc_spatial_norm_bwd_jobs, cc_amd.loss_functions
.normalized_depth_levels).  The inputs are re-creatable from seeds; tools/make_recipe_golden.py writes what the unmodified
reference gives on them into tests/golden/recipe.npz.  Every body expects the engine it should run on to be the current one."""
import os

import numpy as np
import torch

from cc_amd import loss_functions as LF, synthetic as syn, trainer as T

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "recipe.npz")
U = 2.0 ** -24
SB, SH, SW = 2, 128, 192            # the step-level case of oracle/make_golden.py

# (B, C, H, W) per level: less than one workgroup; ragged, four 256-element pieces; an exact multiple of 256 (24 pieces: two
# workgroups per sample, the second half full); C > 1; six elements; one call over the six levels 64x96 ... 2x3
CASES = {
    "7x13": [(2, 1, 7, 13)],
    "33x31": [(3, 1, 33, 31)],
    "64x96": [(2, 1, 64, 96)],
    "c2": [(1, 2, 5, 8)],
    "2x3": [(1, 1, 2, 3)],
    "levels": [(2, 1, 64 >> l, 96 >> l) for l in range(6)],
}
NAMES = list(CASES)
GRADS = ("both", "dn", "depth")
RECIPES = {"a": dict(spatial_normalize=True), "b": dict(no_non_rigid_mask=True), "c": dict(spatial_normalize=True, no_non_rigid_mask=True)}


def inputs(name):
    """-> per level (x, g_dn, g_depth) as float32 numpy arrays: x = 10 * rand + 0.01 (the range of the disparity head), normal
    cotangents.  Seeded by the case's place in CASES and the level."""
    out = []
    for l, shape in enumerate(CASES[name]):
        rs = np.random.RandomState(1000 + 16 * NAMES.index(name) + l)
        x = (10.0 * rs.rand(*shape) + 0.01).astype(np.float32)
        out.append((x, rs.randn(*shape).astype(np.float32), rs.randn(*shape).astype(np.float32)))
    return out


def f64(x, g_dn, g_depth):
    """float64 evaluation of m = mean(x_b), dn = x / m, depth = 1 / dn and of the gradient of sum(g_dn dn) + sum(g_depth depth);
    a cotangent may be None.  -> dict(dn, depth, gx, scale): scale_i = (A_i + mean_j(A_j dn_j)) / m with A = |g_dn| + |g_depth|
    depth^2, what the rounding errors of the fp32 gradient are proportional to (h_i - s / N cancels: a relative bar is wrong)."""
    x = x.astype(np.float64)
    ax = (1, 2, 3)
    m = x.mean(axis=ax, keepdims=True)
    dn = x / m
    depth = 1.0 / dn
    gd = np.zeros_like(x) if g_dn is None else g_dn.astype(np.float64)
    gp = np.zeros_like(x) if g_depth is None else g_depth.astype(np.float64)
    h = gd - gp * depth * depth
    gx = (h - (h * dn).mean(axis=ax, keepdims=True)) / m
    A = np.abs(gd) + np.abs(gp) * depth * depth
    return dict(dn=dn, depth=depth, gx=gx, scale=(A + (A * dn).mean(axis=ax, keepdims=True)) / m)


def run(levels, dev, which="both"):
    """normalized_depth_levels on the levels' x and its backward with the cotangents `which` names -> per level (dn, depth, gx)"""
    xs = [torch.from_numpy(x).to(dev).requires_grad_(True) for x, _, _ in levels]
    dns, dps = LF.normalized_depth_levels(xs)
    outs, cots = [], []
    if which in ("both", "dn"):
        outs += dns
        cots += [torch.from_numpy(g).to(dev) for _, g, _ in levels]
    if which in ("both", "depth"):
        outs += dps
        cots += [torch.from_numpy(g).to(dev) for _, _, g in levels]
    gxs = torch.autograd.grad(outs, xs, cots)
    return [(a.detach().cpu().numpy(), b.detach().cpu().numpy(), c.detach().cpu().numpy()) for a, b, c in zip(dns, dps, gxs)]


def check_forward_against_float64(name, dev):
    levels = inputs(name)
    worst = [0.0, 0.0]
    for (x, _, _), (dn, depth, _) in zip(levels, run(levels, dev)):
        want = f64(x, None, None)
        e_dn = np.abs(dn - want["dn"]) / np.abs(want["dn"])
        e_dp = np.abs(depth - want["depth"]) / np.abs(want["depth"])
        worst = [max(worst[0], float(e_dn.max()) / U), max(worst[1], float(e_dp.max()) / U)]
        print("%s %s: dn %.2f u, depth %.2f u" % (name, x.shape, e_dn.max() / U, e_dp.max() / U))
        assert dn.dtype == np.float32 and depth.dtype == np.float32
        assert np.all(e_dn <= 3 * U), (name, x.shape, float(e_dn.max()) / U)
        assert np.all(e_dp <= 4 * U), (name, x.shape, float(e_dp.max()) / U)
    return worst


def check_backward_against_float64(name, which, dev):
    levels = inputs(name)
    worst = 0.0
    for (x, g_dn, g_dp), (_, _, gx) in zip(levels, run(levels, dev, which)):
        want = f64(x, g_dn if which != "depth" else None, g_dp if which != "dn" else None)
        ratio = np.abs(gx - want["gx"]) / want["scale"]
        worst = max(worst, float(ratio.max()) / U)
        assert np.all(ratio <= 16 * U), (name, which, x.shape, float(ratio.max()) / U)
    print("%s, cotangents %s: worst |gx - gx64| / scale = %.2f u (bar 16 u)" % (name, which, worst))
    return worst


def check_against_reference(name, dev):
    """tests/golden/recipe.npz, function level: the reference's spatial_normalize (and depth = 1 / it) and the gradient of the seeded
    functional.  Bars: what the reference itself was measured to deviate from float64 plus the kernel's own bound (3 u, 4 u, 16 u)."""
    g = np.load(FIXTURE)
    levels = inputs(name)
    for l, ((x, g_dn, g_dp), (dn, depth, gx)) in enumerate(zip(levels, run(levels, dev))):
        k = "fn.%s.%d." % (name, l)
        for got, key, own in ((dn, "dn", 3), (depth, "depth", 4)):
            ref, dist = g[k + key], float(g[k + key + ".ref_vs_f64"])
            assert ref.dtype == np.float32 and ref.shape == got.shape
            err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
            assert np.all(err <= (dist + own * U) * np.abs(ref.astype(np.float64))), (k + key, float((err / np.abs(ref)).max()) / U, dist / U)
        ref, dist = g[k + "gx"], float(g[k + "gx.ref_vs_f64"])
        scale = f64(x, g_dn, g_dp)["scale"]
        err = np.abs(gx.astype(np.float64) - ref.astype(np.float64))
        assert np.all(err <= (dist + 16 * U) * scale), (k + "gx", float((err / scale).max()) / U, dist / U)


def check_reproducible(dev):
    """two calls: equal bits; a level called alone: the bits of its row in the six-level call (forward and backward)"""
    levels = inputs("levels")
    a, b = run(levels, dev), run(levels, dev)
    for ra, rb in zip(a, b):
        assert all(np.array_equal(p, q) for p, q in zip(ra, rb))
    for l, lv in enumerate(levels):
        alone = run([lv], dev)[0]
        assert all(np.array_equal(p, q) for p, q in zip(alone, a[l])), l
    for name in ("33x31", "c2"):
        p, q = run(inputs(name), dev, "depth"), run(inputs(name), dev, "depth")
        assert all(np.array_equal(s, t) for ra, rb in zip(p, q) for s, t in zip(ra, rb))


def check_levels_surface(dev):
    """spatial_normalize_levels = the dn half of normalized_depth_levels; without a gradient to send, no backward launch"""
    levels = inputs("levels")
    xs = [torch.from_numpy(x).to(dev).requires_grad_(True) for x, _, _ in levels]
    dn = LF.spatial_normalize_levels(xs)
    both = LF.normalized_depth_levels(xs)
    assert len(dn) == len(xs) and all(torch.equal(p, q) for p, q in zip(dn, both[0]))
    # a gradient for one level only: the others' inputs get none (absent slots, not zeros)
    gx = torch.autograd.grad([both[1][2]], xs, [torch.ones_like(both[1][2])], allow_unused=True)
    assert [g is not None for g in gx] == [False, False, True, False, False, False]


# ----------------------------------------------------------------------------- the step
def step_batch(dev):
    bc = syn.sample(SB, SH, SW, seed=1)
    return (bc[0].to(dev), [r.to(dev) for r in bc[1]], bc[2].to(dev), bc[3].to(dev))


def seeded_nets(dev, **kw):
    nets = T.build_nets(dev, init=False, **kw)
    for n in nets:
        if n is not None:
            n.load_state_dict(syn.seeded_state_dict(n, 0))
            n.train()
    return nets


def check_step_against_reference(recipe, use_graph, dev):
    """The bars test_full_step_against_reference_golden (tests/test_nets_gpu.py) holds the default recipe to, against the recipe's
    entries of tests/golden/recipe.npz; for the recipes without the non-rigid mask, no complement-slice launch (ops 3, 4)."""
    from loss_calls import ArgLog
    g = np.load(FIXTURE)
    pre = recipe + "."
    batch = step_batch(dev)
    nets = seeded_nets(dev)
    tr = T.CCTrainer(nets, T.StepConfig(**RECIPES[recipe]), use_graph=use_graph)
    with ArgLog() as log:
        got = {k: float(v) for k, v in tr.step(batch).items()}
    for k in ("loss", "loss_1", "loss_2", "loss_3", "loss_4", "loss_5"):
        want = float(g[pre + k])
        print("recipe %s %s: %.8f, reference %.8f, rel %.2e" % (recipe, k, got[k], want, abs(got[k] - want) / abs(want)))
        assert abs(got[k] - want) <= 1e-4 * abs(want), (k, got[k], want)
    names = [c[0] for c in log.calls]
    assert ("cc_spatial_norm_fwd_jobs" in names) == ("cc_spatial_norm_bwd_jobs" in names) == bool(RECIPES[recipe].get("spatial_normalize"))
    ops = [c[1][3] for c in log.calls if c[0] == "cc_elementwise_jobs"]
    if RECIPES[recipe].get("no_non_rigid_mask"):
        assert 3 not in ops and 4 not in ops, ops
    else:
        assert 3 in ops and 4 in ops, ops
    for name, v in tr.grad_norms().items():
        want = float(g[pre + "gradnorm." + name])
        assert abs(float(v) - want) <= 1e-3 * want, (name, float(v), want)
    worst, offs = (0.0, ""), iter(tr.opt.offsets)
    for name, n in zip(("disp", "pose", "mask", "flow"), nets):
        for pn, p in n.named_parameters():
            k, off = p.numel(), next(offs)
            key = pre + "grad.%s.%s" % (name, pn)
            if key in g:
                gw = torch.from_numpy(g[key]).double().reshape(-1)
                gg = tr.opt.flat_g[off:off + k].detach().cpu().double()
                r = float((gg - gw).norm()) / (float(gw.norm()) + 1e-12)
                worst = max(worst, (r, key))
                assert r <= 1e-2, (key, r)
    assert worst[1], "the fixture stores small-parameter gradients"
    print("recipe %s: worst small-parameter gradient mismatch vs the reference: %.2e (%s)" % ((recipe,) + worst))
    got2 = {k: float(v) for k, v in tr.step(batch).items()}
    want2 = float(g[pre + "loss_after_adam"])
    assert abs(got2["loss"] - want2) <= 1e-4 * abs(want2), (got2["loss"], want2)


class _Normalized(torch.nn.Module):
    """train.py:454-456 around an oracle DispResNet6: its disparities, each divided by its per-sample mean"""

    def __init__(self, net):
        super().__init__()
        self.net = net

    def forward(self, x):
        return [d / d.mean(dim=(1, 2, 3), keepdim=True) for d in self.net(x)]


def check_config2_against_oracle(dev):
    """DispResNet6 + PoseNetB6 alone (mask_net / flow_net None) with spatial_normalize, against the oracle's step in float64 with the
    wrapped DispResNet6, at the bar of test_config2_against_reference_golden (1e-4)."""
    from oracle import step as S
    bc = syn.sample(SB, SH, SW, seed=1)
    nets = seeded_nets(dev, flow=False, mask=False)
    out = T.cc_forward(nets, step_batch(dev), T.StepConfig(spatial_normalize=True), keep=True)
    onets = S.build_nets("oracle", flow=False, mask=False)
    for n in onets:
        if n is not None:
            n.load_state_dict(syn.seeded_state_dict(n, 0))
            n.double().train()
    onets[0] = _Normalized(onets[0])
    b64 = (bc[0].double(), [r.double() for r in bc[1]], bc[2].double(), bc[3].double())
    want = S.cc_forward(onets, b64, S.StepConfig(), keep=True)
    for k in ("loss", "loss_1", "loss_3"):
        a, b = float(out[k].detach()), float(want[k].detach())
        print("config 2, spatial_normalize, %s: %.8f, float64 oracle %.8f, rel %.2e" % (k, a, b, abs(a - b) / abs(b)))
        assert abs(a - b) <= 1e-4 * abs(b), (k, a, b)
    # keep=True hands back the NORMALISED disparities (what train.py logs): per-sample mean 1
    for d in out["disparities"]:
        assert float((d.detach().double().mean(dim=(1, 2, 3)) - 1).abs().max()) <= 4 * U


def check_explicit_defaults_change_no_bit(dev):
    """The loss phase of tests/loss_calls.py (seeded stand-ins for the networks' outputs) with both fields named and False: the
    launches, losses and gradients of the phase built without naming them, bit for bit."""
    import loss_calls as LC
    la, ga, ca = LC.loss_phase(dev)
    orig = T.StepConfig
    T.StepConfig = lambda **kw: orig(spatial_normalize=False, no_non_rigid_mask=False, **kw)
    try:
        lb, gb, cb = LC.loss_phase(dev)
    finally:
        T.StepConfig = orig
    assert ca == cb and not any(c[0].startswith("cc_spatial_norm") for c in ca)
    assert la.keys() == lb.keys() and all(torch.equal(la[k], lb[k]) for k in la)
    assert all((p is None and q is None) or torch.equal(p, q) for p, q in zip(ga, gb))


def check_argument_errors(dev):
    """a table the entry points cannot run is CC_ERR_ARG before anything is launched"""
    import ctypes
    from cc_amd._lib import engine, STREAM
    E = engine()
    x = torch.ones(2, 1, 4, 4, device=dev)
    m = torch.empty(2, device=dev)
    part = torch.empty(2, device=dev, dtype=torch.float64)
    assert E.call("cc_spatial_norm_pieces", 1) == 1 and E.call("cc_spatial_norm_pieces", 4096) == 1
    assert E.call("cc_spatial_norm_pieces", 4097) == 2 and E.call("cc_spatial_norm_pieces", 0) == 0

    def table(rows):
        arr = (ctypes.c_long * (10 * len(rows)))()
        for j, (slots, H, W) in enumerate(rows):
            for k, v in enumerate(slots):
                arr[10 * j + k] = 0 if v is None else v.data_ptr()
            arr[10 * j + 8], arr[10 * j + 9] = H, W
        return arr

    def refused(name, rows, njobs=None, B=2):
        arr = table(rows)
        try:
            E.call(name, ctypes.addressof(arr), len(rows) if njobs is None else njobs, B, STREAM)
        except RuntimeError as err:
            return "failed with code" in str(err)
        return False
    ok = [x, x.clone(), x.clone(), m, part]
    assert refused("cc_spatial_norm_fwd_jobs", [(ok, 4, 4)], njobs=0)
    assert refused("cc_spatial_norm_fwd_jobs", [(ok, 4, 4)] * 25)
    assert refused("cc_spatial_norm_fwd_jobs", [(ok, 4, 4)], B=0)
    assert refused("cc_spatial_norm_fwd_jobs", [(ok, 0, 4)])
    assert refused("cc_spatial_norm_fwd_jobs", [(ok, 1 << 16, 1 << 15)])
    for k in (0, 3, 4):                                   # x, m, partials
        assert refused("cc_spatial_norm_fwd_jobs", [(ok[:k] + [None] + ok[k + 1:], 4, 4)]), k
    okb = [x, x.clone(), x.clone(), x.clone(), m, x.clone(), part]
    assert refused("cc_spatial_norm_bwd_jobs", [([None, None] + okb[2:], 4, 4)])
    for k in (2, 3, 4, 5, 6):                             # dn, depth, m, gx, partials
        assert refused("cc_spatial_norm_bwd_jobs", [(okb[:k] + [None] + okb[k + 1:], 4, 4)]), k
    assert not refused("cc_spatial_norm_fwd_jobs", [(ok, 4, 4)])


# ----------------------------------------------------------------------------- the step's forms (MI355X)
def _three_steps(tr, batch):
    ls = [{k: float(v) for k, v in tr.step(batch).items()} for _ in range(3)]
    assert all(np.isfinite(v) for l in ls for v in l.values()), ls
    assert ls[0]["loss"] != ls[1]["loss"] != ls[2]["loss"], ls          # (the weights moved between the replays)
    return ls


def check_step_forms_agree(deterministic, monkeypatch, dev):
    """test_step_forms_agree (tests/test_nets_gpu.py) with spatial_normalize: "post", "staged" and "per_network" as captured graphs:
    same losses, gradients and parameters over three steps -- bit for bit with config.deterministic, to 1e-4 of the gradient norm
    with float atomics."""
    from cc_amd import config
    monkeypatch.setattr(config, "deterministic", deterministic)
    batch = step_batch(dev)
    res = []
    for form in ("post", "staged", "per_network"):
        nets = seeded_nets(dev)
        tr = T.CCTrainer(nets, T.StepConfig(spatial_normalize=True), use_graph=True, pipeline=form)
        l1 = {k: float(v) for k, v in tr.step(batch).items()}
        g1 = tr.opt.flat_g.clone()
        l2 = {k: float(v) for k, v in tr.step(batch).items()}
        l3 = {k: float(v) for k, v in tr.step(batch).items()}
        assert all(np.isfinite(v) for l in (l1, l2, l3) for v in l.values())
        assert l1["loss"] != l2["loss"] and l2["loss"] != l3["loss"]      # three replays: finite, changing losses
        assert tr.pipeline == form and float(tr.opt.step_dev) == 3.0 and (tr.graph_b is not None) == (form == "staged")
        res.append((l1, g1, l2, l3, tr.opt.flat_p.clone()))
        offs = iter(tr.opt.offsets)         # (name, first element, elements) of every parameter tensor in the bucket: the same in all forms
        where = [("%s.%s" % (nm, pn), next(offs), p.numel()) for nm, n in zip(T.NET_NAMES, nets) for pn, p in n.named_parameters()]

    def tensors(x, y):
        """the parameter tensors in which two buckets differ: (name, elements that differ, largest difference)"""
        return [(name, int((x[o:o + k] != y[o:o + k]).sum()), float((x[o:o + k] - y[o:o + k]).abs().max()))
                for name, o, k in where if not torch.equal(x[o:o + k], y[o:o + k])]
    a1, ga, a2, a3, pa = res[0]
    bad = []
    for form, (b1, gb, b2, b3, pb) in zip(("staged", "per_network"), res[1:]):
        for k in a1:
            assert abs(a1[k] - b1[k]) <= 1e-6 * abs(a1[k]) + 1e-9, (k, a1[k], b1[k])
            assert abs(a2[k] - b2[k]) <= 1e-5 * abs(a2[k]) + 1e-9, (k, a2[k], b2[k])
            assert abs(a3[k] - b3[k]) <= 2e-5 * abs(a3[k]) + 1e-9, (k, a3[k], b3[k])
        if deterministic:
            if not torch.equal(ga, gb):
                t = tensors(ga, gb)
                bad.append((form, "gradient of step 1", len(t), t[:12]))
            if not torch.equal(pa, pb):
                bad.append((form, "parameters after step 3", len(tensors(pa, pb))))
            bad += [(form, n, x, y) for n, x, y in (("step 1", a1, b1), ("step 2", a2, b2), ("step 3", a3, b3)) if x != y]
            continue
        assert float((ga - gb).norm() / ga.norm()) < 1e-4
        assert float((pa - pb).abs().max()) <= 3 * 2.001e-4
    assert not bad, bad          # ("post" is the form the other two are compared with)


def check_switch_changes_no_bit(switch, use_graph, monkeypatch, dev):
    """test_loss_phase_on_two_streams_changes_no_bit (switch "loss_stream") and test_network_streams_change_nothing_but_the_schedule
    (switch "net_streams") of tests/test_nets_gpu.py with spatial_normalize: three deterministic steps with the switch off and on
    give identical losses, gradient bucket and parameters."""
    from cc_amd import config
    monkeypatch.setattr(config, "deterministic", True)
    batch = step_batch(dev)
    res = []
    for on in (False, True):
        monkeypatch.setattr(config, switch, on)
        nets = seeded_nets(dev)
        tr = T.CCTrainer(nets, T.StepConfig(spatial_normalize=True), use_graph=use_graph)
        assert bool(tr.net_streams) == (on if switch == "net_streams" else True)
        res.append((_three_steps(tr, batch), tr.opt.flat_g.clone(), tr.opt.flat_p.clone()))
    (la, ga, pa), (lb, gb, pb) = res
    assert la == lb
    assert torch.equal(ga, gb) and torch.equal(pa, pb)


def check_explicit_defaults_step(dev, monkeypatch):
    """a whole training step with both fields named and False: the bits of the step built without naming them"""
    from cc_amd import config
    monkeypatch.setattr(config, "deterministic", True)
    batch = step_batch(dev)
    res = []
    for kw in ({}, dict(spatial_normalize=False, no_non_rigid_mask=False)):
        tr = T.CCTrainer(seeded_nets(dev), T.StepConfig(**kw), use_graph=False)
        res.append(({k: float(v) for k, v in tr.step(batch).items()}, tr.opt.flat_g.clone(), tr.opt.flat_p.clone()))
    assert res[0][0] == res[1][0] and torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])


def check_capture_stream(monkeypatch, dev):
    tr = T.CCTrainer(seeded_nets(dev), T.StepConfig(), use_graph=True)
    assert tr.net_streams and len(tr.net_streams) == 2
    real, handed = torch.cuda.Stream, []
    pending = list(tr.net_streams)              # what the pool would hand out next, had it wrapped round to them

    def stream(*a, **kw):
        handed.append(pending.pop(0) if pending else real(*a, **kw))
        return handed[-1]
    monkeypatch.setattr(torch.cuda, "Stream", stream)
    s = tr._capture_stream()
    monkeypatch.setattr(torch.cuda, "Stream", real)
    taken = {st.cuda_stream for st in tr.net_streams} | {torch.cuda.current_stream().cuda_stream}
    assert len(handed) == 3 and s is handed[2] and s.cuda_stream not in taken
    # and the capture uses it: during the captured step the current stream is none of the networks' streams
    seen = []
    orig = tr._step_pipelined
    monkeypatch.setattr(tr, "_step_pipelined", lambda b: (seen.append(torch.cuda.current_stream().cuda_stream), orig(b))[1])
    tr.step(step_batch(dev))
    assert len(seen) == 3 and not set(seen) & {st.cuda_stream for st in tr.net_streams}      # two warm-ups and the capture
