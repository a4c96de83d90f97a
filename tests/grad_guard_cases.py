"""The gradient guard of the in-graph Adam step (cc_grad_sumsq / cc_grad_guard_finish / cc_adam_step_segment_guard, FlatAdam's
guard table): the cases shared by tests/test_grad_guard.py (x86 emulation build, CPU tensors) and tests/test_grad_guard_gpu.py
(the product library).  torch.nn.utils.clip_grad_norm_ + torch.optim.Adam are the reference."""
import ctypes

import pytest
import torch

from cc_amd import trainer as T
from cc_amd._lib import engine, STREAM
from optim_hyper_cases import BOUNDS, OFF, ROWS, _state, _sync

INF = float("inf")
SCALE = 0.5
NB_MAX = T.FlatAdam.GUARD_BLOCKS
SWEEP = NB_MAX * 256 * 4 * 4        # floats one turn of cc_grad_sumsq's unrolled loop covers at the full grid (4 float4 per work-item)
# 64: one workgroup, most work-items idle; 3 * 1024 + 7: one workgroup, remainder loop + 3 tail elements; the last: full grid, every
# work-item takes the unrolled turn once, 517 of them one more float4 in the remainder loop, one tail element
NORM_SIZES = [64, 3 * 1024 + 7, SWEEP + 4 * 517 + 1]


def _row(h, max_norm):
    return [h[0], h[1], h[2], h[3], h[4], max_norm, 0.0, 0.0]


def guard_row(g, hyper_row, dev, scale=SCALE, guard=None):
    """cc_grad_sumsq + cc_grad_guard_finish on g -> (the guard row, the grid).  The partials start as NaN: nothing clears them, every
    one the finish reads has to have been written by this call."""
    partials = torch.full((NB_MAX,), float("nan"), dtype=torch.float64).to(dev)
    guard = torch.zeros(8, dtype=torch.float32).to(dev) if guard is None else guard
    nb = ctypes.c_int(0)
    engine().call("cc_grad_sumsq", g, g.numel(), partials, ctypes.addressof(nb), STREAM)
    engine().call("cc_grad_guard_finish", partials, nb.value, hyper_row, scale, guard, STREAM)
    return guard, nb.value


def norm_case(n, dev, spike=False):
    """-> (guard row of a first call, of a second call on the same gradient, grad_scale * ||g|| in fp64, the grid)"""
    g = _state(n, dev, 5, OFF)[1]
    if spike:
        g[OFF + n // 2] = 1e25          # its square overflows fp32
    view = g[OFF:]                      # base pointer 64 floats into the allocation
    hyper = torch.tensor(_row(ROWS[0], INF), dtype=torch.float32).to(dev)
    a, nb = guard_row(view, hyper, dev)
    b, _ = guard_row(view, hyper, dev)
    _sync(dev)
    return a.cpu(), b.cpu(), SCALE * float(g[OFF:].double().norm()), nb


def grads(dev, steps=3):
    return [_state(BOUNDS[-1], dev, 10 + k)[1] for k in range(steps)]


def max_norms(g0):
    """(half row 0's norm, ten times row 1's norm, inf) from the first step's gradient as Adam consumes it"""
    nrm = [SCALE * float(g0[lo:hi].double().norm()) for lo, hi in zip(BOUNDS, BOUNDS[1:])]
    return [0.5 * nrm[0], 10.0 * nrm[1], INF]


def guarded_steps(dev, gs, mx):
    """Three rows over BOUNDS with ROWS' hyperparameters and max_grad_norm mx, from zero moments, one step per gradient of gs: the
    counter ticks once per step, every row runs sumsq -> finish -> guarded Adam.
    -> per step {"p", "m", "v", "guard" [3, 8], "step"} (clones)"""
    n = BOUNDS[-1]
    table = torch.tensor([_row(h, x) for h, x in zip(ROWS, mx)], dtype=torch.float32).to(dev)
    p = _state(n, dev, 3)[0]
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    step = torch.zeros(1, dtype=torch.float32).to(dev)
    guard = torch.zeros(len(ROWS), 8, dtype=torch.float32).to(dev)
    out = []
    for g in gs:
        engine().call("cc_adam_tick", step, STREAM)
        for k, (lo, hi) in enumerate(zip(BOUNDS, BOUNDS[1:])):
            guard_row(g[lo:hi], table[k], dev, guard=guard[k])
            engine().call("cc_adam_step_segment_guard", p[lo:hi], g[lo:hi], m[lo:hi], v[lo:hi], step, hi - lo, table[k], guard[k],
                          SCALE, STREAM)
        _sync(dev)
        out.append({"p": p.clone(), "m": m.clone(), "v": v.clone(), "guard": guard.clone().cpu(), "step": float(step)})
    return out


def hyper_steps(dev, gs):
    """the same rows through cc_adam_step_segment_hyper (no guard) -> [p, m, v] after the last step"""
    n = BOUNDS[-1]
    table = torch.tensor([_row(h, 0.0) for h in ROWS], dtype=torch.float32).to(dev)
    p = _state(n, dev, 3)[0]
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    step = torch.zeros(1, dtype=torch.float32).to(dev)
    for g in gs:
        for k, (lo, hi) in enumerate(zip(BOUNDS, BOUNDS[1:])):
            engine().call("cc_adam_step_segment_hyper", p[lo:hi], g[lo:hi], m[lo:hi], v[lo:hi], step, hi - lo, table[k], SCALE,
                          int(k == 0), STREAM)
    _sync(dev)
    return [p, m, v]


def torch_steps(dev, dtype, gs, mx, no_grad=()):
    """clip_grad_norm_ + torch.optim.Adam per slice; (step, row) in no_grad: that group has grad = None in that step
    -> the parameters after the last step"""
    p0 = _state(BOUNDS[-1], dev, 3)[0].to(dtype)
    ref = [p0[lo:hi].clone().requires_grad_(True) for lo, hi in zip(BOUNDS, BOUNDS[1:])]
    topt = torch.optim.Adam([{"params": [q], "lr": h[0], "betas": (h[1], h[2]), "eps": h[3], "weight_decay": h[4]}
                             for q, h in zip(ref, ROWS)])
    for s, g in enumerate(gs):
        for k, (q, (lo, hi)) in enumerate(zip(ref, zip(BOUNDS, BOUNDS[1:]))):
            if (s, k) in no_grad:
                q.grad = None
                continue
            q.grad = g[lo:hi].to(dtype) * SCALE
            torch.nn.utils.clip_grad_norm_([q], mx[k])
        topt.step()
    return torch.cat([q.detach() for q in ref])


def poisoned(g):
    """a NaN as the LAST element of row 1 (the end of a float4) and a +Inf as the last element of row 2 (its scalar tail)"""
    g = g.clone()
    g[BOUNDS[2] - 1] = float("nan")
    g[BOUNDS[3] - 1] = INF
    return g


# ---------------------------------------------------------------------------------------------------------------- FlatAdam
def four_nets(dev):
    torch.manual_seed(0)
    return [torch.nn.Sequential(torch.nn.Linear(3 + k, 5), torch.nn.Linear(5, 2)).to(dev) for k in range(4)]


class CallLog:
    """the names of the engine calls made inside the block"""

    def __enter__(self):
        self.e, self.names = engine(), []
        self.orig = self.e.call

        def call(name, *a):
            self.names.append(name)
            return self.orig(name, *a)
        self.e.call = call
        return self

    def __exit__(self, *a):
        del self.e.call
        return False


def backward(opt, nets, dev, seed, poison=None):
    """a fresh gradient in the bucket; poison: a network index whose gradient gets a NaN"""
    gen = torch.Generator().manual_seed(seed)
    opt.zero_grad()
    sum(n(torch.randn(2, 3 + k, generator=gen).to(dev)).pow(2).sum() for k, n in enumerate(nets)).backward()
    if poison is not None:
        lo, hi = opt.net_ranges[poison]
        opt.flat_g[hi - 1] = float("nan")


# ------------------------------------------------------------------------------------------ the checks, on either device
def check_norm(n, dev):
    a, b, want, nb = norm_case(n, dev)
    assert nb == min(NB_MAX, -(-n // 4096))
    rel = abs(float(a[0]) - want) / want
    print("n = %d (%d workgroups): norm %.9g, fp64 %.9g, rel %.2e" % (n, nb, float(a[0]), want, rel))
    # fp64 accumulation: what is left is the rounding of the result to fp32 (6e-8)
    assert rel < 1e-6, (n, float(a[0]), want)
    assert a.tolist()[1:] == [1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0]             # coef (max_grad_norm = inf), finite, skipped, zeros
    assert torch.equal(a, b), "two calls on the same gradient differ"
    # one element at 1e25: its square overflows fp32, the fp64 sum does not
    a, b, want, _ = norm_case(n, dev, spike=True)
    assert want > 1e24 and abs(float(a[0]) - want) / want < 1e-6 and float(a[2]) == 1.0 and float(a[1]) == 1.0 and float(a[3]) == 0.0
    assert torch.equal(a, b)


def check_clip_against_torch(dev):
    gs = grads(dev)
    mx = max_norms(gs[0])
    ours = guarded_steps(dev, gs, mx)
    t32, t64 = torch_steps(dev, torch.float32, gs, mx), torch_steps(dev, torch.float64, gs, mx)
    for s in ours:
        coef = s["guard"][:, 1].tolist()
        assert 0.4 < coef[0] < 0.6 and coef[1] == 1.0 and coef[2] == 1.0, coef
        assert s["guard"][:, 2].tolist() == [1.0] * 3 and s["guard"][:, 3].tolist() == [0.0] * 3
    assert ours[-1]["step"] == 3.0
    ref_err = float((t32.double() - t64).abs().max())
    for lo, hi in zip(BOUNDS, BOUNDS[1:]):
        d = float((ours[-1]["p"][lo:hi] - t32[lo:hi]).abs().max())
        print("rows [%d, %d): max |guarded kernel - clip_grad_norm_ + torch.optim.Adam| = %.3e (torch fp32 vs fp64 %.3e)" % (lo, hi, d, ref_err))
        assert d < 1e-6, (lo, hi, d)
    assert ref_err < 1e-6, ref_err
    # coef == 1, skipped == 0: the unguarded entry's bits
    plain = hyper_steps(dev, gs)
    lo, hi = BOUNDS[1], BOUNDS[3]
    for k, t in zip("pmv", plain):
        assert torch.equal(ours[-1][k][lo:hi], t[lo:hi]), k
    assert not torch.equal(ours[-1]["p"][:lo], plain[0][:lo])                 # (row 0 was clipped)


def check_skip(dev):
    gs = grads(dev)
    mx = max_norms(gs[0])
    s1, s2, s3 = guarded_steps(dev, gs[:1] + [poisoned(gs[1])] + gs[2:], mx)
    lo, hi = BOUNDS[1], BOUNDS[3]
    for k in "pmv":
        assert torch.equal(s2[k][lo:hi], s1[k][lo:hi]), k                     # rows 1, 2: not a bit moved
        assert not torch.equal(s2[k][:lo], s1[k][:lo]), k                     # row 0 moved
        assert bool(torch.isfinite(s2[k]).all())
    g2 = s2["guard"]
    assert g2[:, 2].tolist() == [1.0, 0.0, 0.0] and g2[:, 1].tolist()[1:] == [0.0, 0.0] and g2[:, 3].tolist() == [0.0, 1.0, 1.0]
    assert 0.0 < float(g2[0, 1]) < 1.0
    assert s3["guard"][:, 2].tolist() == [1.0] * 3 and s3["guard"][:, 3].tolist() == [0.0, 1.0, 1.0] and s3["step"] == 3.0
    # torch.optim.Adam whose groups 1 and 2 had grad = None in step 2
    t32 = torch_steps(dev, torch.float32, gs, mx, no_grad={(1, 1), (1, 2)})
    t64 = torch_steps(dev, torch.float64, gs, mx, no_grad={(1, 1), (1, 2)})
    d, ref_err = float((s3["p"] - t32).abs().max()), float((t32.double() - t64).abs().max())
    print("after the skipped step: max |guarded - torch| = %.3e (torch fp32 vs fp64 %.3e)" % (d, ref_err))
    assert d < 1e-6 and ref_err < 1e-6, (d, ref_err)
    # ... and the bits of a run that never saw step 2: counter 2 against 3, skipped 0 against 1
    never = guarded_steps(dev, [gs[0], gs[2]], mx)[-1]
    assert never["step"] == 2.0 and never["guard"][:, 3].tolist() == [0.0] * 3
    for k in "pmv":
        assert torch.equal(s3[k][lo:hi], never[k][lo:hi]), k


def check_guard_off_surface(dev):
    nets = four_nets(dev)
    opt = T.FlatAdam(nets, T.StepConfig(lr=2e-4, weight_decay=1e-2, eps=1e-7))
    assert not opt.guard and opt.guard_dev is None
    assert opt.hyper_of("pose") == {"lr": 2e-4, "betas": (0.9, 0.999), "eps": 1e-7, "weight_decay": 1e-2}
    assert opt.state_dict()["param_groups"][0] == {"lr": 2e-4, "betas": (0.9, 0.999), "eps": 1e-7, "weight_decay": 1e-2,
                                                   "amsgrad": False, "params": list(range(16))}
    assert list(opt.param_groups[0]) == ["lr", "betas", "eps", "weight_decay", "amsgrad", "params"]
    with pytest.raises(ValueError):
        opt.set_hyper("disp", max_grad_norm=1.0)
    with pytest.raises(ValueError):
        opt.set_hyper(max_grad_norm=INF)
    with pytest.raises(KeyError):
        opt.param_groups[0]["max_grad_norm"] = 1.0
    with pytest.raises(ValueError):
        opt.grad_stats()
    backward(opt, nets, dev, 1)
    with CallLog() as log:
        opt.step()
        opt.step_segment(0, opt.segment(2)[0], True)
    assert log.names == ["cc_adam_step_hyper"] + ["cc_adam_step_segment_hyper"] * 2
    assert float(opt.hyper_dev[:, 5:].abs().max()) == 0.0 and float(opt.step_dev) == 2.0
    sd = opt.state_dict()
    assert float(sd["state"][0]["step"]) == 2.0 and "max_grad_norm" not in sd["param_groups"][0]


def check_guard_on_surface(dev):
    nets = four_nets(dev)
    opt = T.FlatAdam(nets, T.StepConfig(max_grad_norm=INF))
    assert opt.guard and tuple(opt.guard_dev.shape) == (4, 8) and len({t.data_ptr() for t in opt._partials}) == 4
    assert opt.hyper_of("mask") == {"lr": 1e-4, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0.0, "max_grad_norm": INF}
    opt.set_hyper("disp", max_grad_norm=0.25)
    opt.param_groups[3]["max_grad_norm"] = 2.0
    assert opt.hyper_of(0)["max_grad_norm"] == 0.25 and opt.param_groups[0]["max_grad_norm"] == 0.25
    assert opt.hyper_of("flow")["max_grad_norm"] == 2.0 and opt.hyper_of("pose")["max_grad_norm"] == INF
    assert "max_grad_norm" in list(opt.param_groups[0])
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            opt.set_hyper("pose", max_grad_norm=bad)
    opt.flush_hyper()
    assert opt.hyper_dev[:, 5].tolist() == [0.25, INF, INF, 2.0] and float(opt.hyper_dev[:, 6:].abs().max()) == 0.0
    # a partial row: its norm is not known
    lo, hi = opt.segment(1)
    for a, b in ((lo, hi - 4), (lo + 4, hi), (0, lo + 4)):
        with pytest.raises(ValueError):
            opt.step_segment(a, b, False)
    assert float(opt.step_dev) == 0.0
    # step 1 clean, step 2 with a NaN in PoseNet's gradient, step 3 clean -- one as step(), one as whole-row ranges
    backward(opt, nets, dev, 1)
    with CallLog() as log:
        opt.step()
    assert log.names == ["cc_adam_tick"] + ["cc_grad_sumsq", "cc_grad_guard_finish", "cc_adam_step_segment_guard"] * 4
    st = opt.grad_stats(sync=True)
    assert list(st) == ["disp", "pose", "mask", "flow"] and all(v["finite"] == 1.0 and v["skipped"] == 0.0 for v in st.values())
    assert 0.0 < st["disp"]["coef"] < 1.0 and st["pose"]["coef"] == 1.0 and st["disp"]["norm"] > 0.25
    want = float(opt.flat_g[slice(*opt.segment(0))].double().norm())
    assert abs(st["disp"]["norm"] - want) < 1e-6 * want
    assert torch.is_tensor(opt.grad_stats()["flow"]["norm"]) and opt.grad_stats()["flow"]["norm"].dim() == 0
    before = [t.clone() for t in (opt.flat_p, opt.exp_avg, opt.exp_avg_sq)]
    backward(opt, nets, dev, 2, poison=1)
    opt.step_segment(0, opt.segment(2)[0], True)
    opt.step_segment(opt.segment(2)[0], None, False)
    for t, t0 in zip((opt.flat_p, opt.exp_avg, opt.exp_avg_sq), before):
        assert torch.equal(t[lo:hi], t0[lo:hi]) and not torch.equal(t[:lo], t0[:lo]) and not torch.equal(t[hi:], t0[hi:])
    st = opt.grad_stats(sync=True)
    assert [v["skipped"] for v in st.values()] == [0.0, 1.0, 0.0, 0.0] and st["pose"]["finite"] == 0.0 and st["pose"]["coef"] == 0.0
    backward(opt, nets, dev, 3)
    opt.step()
    assert float(opt.step_dev) == 3.0
    # state_dict: per-network steps, max_grad_norm in the groups; a torch.optim.Adam with the same groups loads it
    sd = opt.state_dict()
    assert [float(sd["state"][i]["step"]) for i in (0, 4, 8, 12)] == [3.0, 2.0, 3.0, 3.0]
    assert [g["max_grad_norm"] for g in sd["param_groups"]] == [0.25, INF, INF, 2.0]
    tnets = four_nets(dev)
    topt = torch.optim.Adam([{"params": list(n.parameters())} for n in tnets])
    topt.load_state_dict(sd)
    assert float(topt.state[next(tnets[1].parameters())]["step"]) == 2.0
    assert float(topt.state[next(tnets[3].parameters())]["step"]) == 3.0
    # load_state_dict: counter = the largest step, skipped = what a network is behind it, max_grad_norm from the groups
    opt2 = T.FlatAdam(four_nets(dev), T.StepConfig(max_grad_norm=1.0))
    opt2.load_state_dict(topt.state_dict())
    assert float(opt2.step_dev) == 3.0 and opt2.guard_dev[:, 3].tolist() == [0.0, 1.0, 0.0, 0.0]
    assert [opt2.hyper_of(i)["max_grad_norm"] for i in range(4)] == [0.25, INF, INF, 2.0]
    assert torch.equal(opt2.exp_avg, opt.exp_avg) and torch.equal(opt2.exp_avg_sq, opt.exp_avg_sq)
    # ... and the next step of both is the same step (PoseNet at t = 3, the others at t = 4)
    opt2.flat_p.copy_(opt.flat_p)
    for o, ns in ((opt, nets), (opt2, None)):
        if ns is not None:
            backward(o, ns, dev, 4)
        else:
            o.flat_g.copy_(opt.flat_g)
        o.step()
    assert torch.equal(opt2.flat_p, opt.flat_p) and torch.equal(opt2.exp_avg_sq, opt.exp_avg_sq)
    # a file without max_grad_norm (an unguarded run's) keeps the rows' values
    plain = T.FlatAdam(four_nets(dev), T.StepConfig()).state_dict()
    opt2.load_state_dict(plain)
    assert [opt2.hyper_of(i)["max_grad_norm"] for i in range(4)] == [0.25, INF, INF, 2.0]
