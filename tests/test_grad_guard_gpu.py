"""The gradient guard of the Adam step on the MI355X: the three kernels against clip_grad_norm_ + torch.optim.Adam, and the guard
inside a step that was captured into a hipGraph -- free when it has nothing to do, clipping after a set_hyper() without a new
capture, and a non-finite gradient that skips exactly the networks it reached."""
import collections
import math

import pytest
import torch

import grad_guard_cases as C
from cc_amd import config, synthetic as syn, trainer as T

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.mark.parametrize("n", C.NORM_SIZES)
def test_norm_on_device(n):
    C.check_norm(n, DEV)


def test_clip_and_adam_match_torch_on_device():
    C.check_clip_against_torch(DEV)


def test_non_finite_rows_are_left_alone_on_device():
    C.check_skip(DEV)


def test_flat_adam_surface_on_device():
    C.check_guard_off_surface(DEV)
    C.check_guard_on_surface(DEV)


# ------------------------------------------------------------------------------------------------------ the captured step
def _batch(dev):
    bc = syn.sample(2, 128, 192, seed=1)
    return (bc[0].to(dev), [r.to(dev) for r in bc[1]], bc[2].to(dev), bc[3].to(dev))


def _trainer(cfg):
    dev = torch.device("cuda")
    nets = T.build_nets(dev, init=False)
    for n in nets:
        n.load_state_dict(syn.seeded_state_dict(n, 0))
    tr = T.CCTrainer(nets, cfg, use_graph=True)
    assert tr.pipeline == "per_network"
    return tr


def _snapshot(tr, losses=None):
    torch.cuda.synchronize()
    s = {"p": tr.opt.flat_p.clone(), "m": tr.opt.exp_avg.clone(), "v": tr.opt.exp_avg_sq.clone(), "g": tr.opt.flat_g.clone(),
         "step": float(tr.opt.step_dev)}
    if losses is not None:
        s["losses"] = {k: float(x) for k, x in losses.items()}
    return s


@pytest.fixture(scope="module")
def runs():
    """Trainer A (guard off) and trainer B (max_grad_norm = inf): three steps each, the third a replay; then on B a fourth step with
    DispResNet6 clipped to half the norm it just had.  One after the other: ops.packs belongs to the trainer built last."""
    batch = _batch(torch.device("cuda"))
    old = config.deterministic
    config.deterministic = True
    try:
        a = _trainer(T.StepConfig())
        with C.CallLog() as calls_a:
            for _ in range(3):
                la = a.step(batch)
        sa = _snapshot(a, la)
        with pytest.raises(ValueError):
            a.grad_stats()
        del a
        b = _trainer(T.StepConfig(max_grad_norm=C.INF))
        with C.CallLog() as calls_b:
            for _ in range(3):
                lb = b.step(batch)
        sb = _snapshot(b, lb)
        stats = b.grad_stats(sync=True)
        views = b.grad_stats()
        norms = {k: float(v) for k, v in b.grad_norms().items()}
        graph = b.graph
        b.opt.set_hyper("disp", max_grad_norm=0.5 * stats["disp"]["norm"])
        b.step(batch)
        sc = _snapshot(b)
        out = dict(sa=sa, sb=sb, stats=stats, views=views, norms=norms, same_graph=b.graph is graph and graph is not None, sc=sc,
                   stats_c=b.grad_stats(sync=True),
                   calls_a=collections.Counter(calls_a.names), calls_b=collections.Counter(calls_b.names), segs=[b.opt.segment(i) for i in range(4)],
                   hyper=[b.opt.hyper_of(i) for i in range(4)])
        del b
    finally:
        config.deterministic = old
    return out


def test_guard_with_nothing_to_do_changes_nothing(runs):
    sa, sb = runs["sa"], runs["sb"]
    assert sa["losses"] == sb["losses"], (sa["losses"], sb["losses"])
    assert sa["step"] == sb["step"] == 3.0
    for k in ("p", "m", "v"):
        assert torch.equal(sa[k], sb[k]), (k, float((sa[k] - sb[k]).abs().max()))
    for name, st in runs["stats"].items():
        rel = abs(st["norm"] - runs["norms"][name]) / runs["norms"][name]
        print("%s: guard norm %.9g, ATen fp64 %.9g, rel %.2e" % (name, st["norm"], runs["norms"][name], rel))
        assert rel < 1e-6, (name, st["norm"], runs["norms"][name])
        assert st == {"norm": st["norm"], "coef": 1.0, "finite": 1.0, "skipped": 0.0}
        v = runs["views"][name]["norm"]
        assert torch.is_tensor(v) and v.is_cuda and v.dim() == 0


def test_guard_off_issues_no_guard_launch_and_guard_on_only_adds_its_own(runs):
    """the engine calls of capture (two eager warm-up steps + the captured one) and two replays: with the guard off none of the
    guard's entries and the four Adam segments per step; with it on the same calls, each Adam segment replaced by the three guard
    launches"""
    a, b = dict(runs["calls_a"]), dict(runs["calls_b"])
    guard = ("cc_grad_sumsq", "cc_grad_guard_finish", "cc_adam_step_segment_guard")
    assert not any(k in a for k in guard) and a["cc_adam_step_segment_hyper"] == 12 and a["cc_adam_tick"] == 3
    assert all(b.pop(k) == 12 for k in guard) and "cc_adam_step_segment_hyper" not in b
    del a["cc_adam_step_segment_hyper"]
    # cc_conv2d_wgrad_ws_bytes is a host-side size query that launches nothing and that ops._wgrad_ws_bytes memoises per process and
    # geometry: whichever trainer of the process comes first asks, the later ones do not
    for d in (a, b):
        d.pop("cc_conv2d_wgrad_ws_bytes", None)
    assert a == b


def test_clipping_reaches_the_captured_step(runs):
    """set_hyper('disp', max_grad_norm = half its norm) on the captured trainer, one more step: same graph object, DispResNet6's
    coefficient inside (0, 1), the others 1, and every network's p, exp_avg, exp_avg_sq are Adam's formulas on the snapshot with
    flat_g * coef (the bucket holds the unclipped gradient) within 1e-6 absolute"""
    assert runs["same_graph"], "the step was captured again"
    s0, s1, st = runs["sb"], runs["sc"], runs["stats_c"]
    assert 0.0 < st["disp"]["coef"] < 1.0 and all(st[k]["coef"] == 1.0 for k in ("pose", "mask", "flow")), st
    assert all(v["finite"] == 1.0 and v["skipped"] == 0.0 for v in st.values()) and s1["step"] == 4.0
    for name, (lo, hi), h in zip(T.NET_NAMES, runs["segs"], runs["hyper"]):
        want_norm = float(s1["g"][lo:hi].double().norm())
        assert abs(st[name]["norm"] - want_norm) < 1e-6 * want_norm
        if name == "disp":
            want = h["max_grad_norm"] / (st[name]["norm"] + 1e-6)
            assert abs(st[name]["coef"] - want) < 1e-6 * want
        (b1, b2), lr, eps, t = h["betas"], h["lr"], h["eps"], s1["step"]
        g = s1["g"][lo:hi].double() * st[name]["coef"] + h["weight_decay"] * s0["p"][lo:hi].double()
        m = b1 * s0["m"][lo:hi].double() + (1 - b1) * g
        v = b2 * s0["v"][lo:hi].double() + (1 - b2) * g * g
        p = s0["p"][lo:hi].double() - lr / (1 - b1 ** t) * (m / (v.sqrt() / math.sqrt(1 - b2 ** t) + eps))
        for k, x in (("p", p), ("m", m), ("v", v)):
            d = float((s1[k][lo:hi].double() - x).abs().max())
            print("%s %s: max |step - Adam restated in fp64| = %.3e" % (name, k, d))
            assert d < 1e-6, (name, k, d)
        assert not torch.equal(s1["p"][lo:hi], s0["p"][lo:hi])


def test_non_finite_gradient_skips_the_networks_it_reached():
    """w4 = inf: every forward value stays finite, d loss / d l4 = inf makes the gradients of Back2Future (and of MaskNet6 through
    1 - m[:, 1:3]) non-finite; DispResNet6 and PoseNetB6 receive gradients from l1 / l3 / l5 only.  Two steps: skipped == 2 exactly
    for the networks whose segment of the bucket holds a non-finite element; their p, exp_avg, exp_avg_sq keep their bits, the
    others move and stay finite."""
    batch = _batch(torch.device("cuda"))
    old = config.deterministic
    config.deterministic = True
    try:
        c = _trainer(T.StepConfig(w4=C.INF, max_grad_norm=C.INF))
        p0 = c.opt.flat_p.clone()
        c.step(batch)
        c.step(batch)
        torch.cuda.synchronize()
        st = c.grad_stats(sync=True)
        hit = set()
        for i, name in enumerate(T.NET_NAMES):
            lo, hi = c.opt.segment(i)
            bad = not bool(torch.isfinite(c.opt.flat_g[lo:hi]).all())
            assert (st[name]["skipped"] == 2.0) == bad, (name, st[name], bad)
            assert st[name]["finite"] == (0.0 if bad else 1.0) and st[name]["skipped"] in (0.0, 2.0)
            p, m, v = c.opt.flat_p[lo:hi], c.opt.exp_avg[lo:hi], c.opt.exp_avg_sq[lo:hi]
            if bad:
                hit.add(name)
                assert torch.equal(p, p0[lo:hi]) and float(m.abs().max()) == 0.0 and float(v.abs().max()) == 0.0, name
            else:
                assert not torch.equal(p, p0[lo:hi]) and all(bool(torch.isfinite(t).all()) for t in (p, m, v)), name
        assert "flow" in hit and "disp" not in hit, hit
        assert float(c.opt.step_dev) == 2.0
        del c
    finally:
        config.deterministic = old


def test_grad_chunks_with_the_guard_raise_on_device(monkeypatch):
    monkeypatch.setattr(config, "grad_chunks", True)
    nets = T.build_nets(torch.device("cuda"), init=True)
    with pytest.raises(ValueError, match="gradient chunks"):
        T.CCTrainer(nets, T.StepConfig(max_grad_norm=1.0), use_graph=True)
