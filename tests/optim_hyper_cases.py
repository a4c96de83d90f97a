"""The table-driven Adam entries (cc_adam_step_hyper / cc_adam_step_segment_hyper) and FlatAdam's hyperparameter table: the cases
shared by tests/test_optim_hyper.py (x86 emulation build, CPU tensors) and tests/test_optim_hyper_gpu.py (the product library)."""
import torch

from cc_amd import trainer as T
from cc_amd._lib import engine, STREAM

OFF = 64            # the sub-range entries get base pointers 64 floats into their allocations


def _row(lr, b1, b2, eps, wd):
    return [lr, b1, b2, eps, wd, 0.0, 0.0, 0.0]


def _state(n, dev, seed, pad=0):
    """p, g, m, v of n elements behind `pad` unused ones.  p and g at the scale of network weights and their gradients; v >= 0."""
    gen = torch.Generator().manual_seed(seed)
    p = 0.1 * torch.randn(pad + n, generator=gen)
    g = 0.05 * torch.randn(pad + n, generator=gen)
    m = 0.01 * torch.randn(pad + n, generator=gen)
    v = 1e-3 * torch.rand(pad + n, generator=gen)
    return [t.to(dev) for t in (p, g, m, v)]


def _sync(dev):
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()


def old_against_new(n, dev):
    """three ticks of the old entries and of the new ones (one row, weight decay 0) from the same random state -> list of
    (name, old tensor, new tensor) that have to be equal bit for bit"""
    lr, b1, b2, eps, scale = 2e-4, 0.9, 0.999, 1e-8, 0.5
    table = torch.tensor([_row(lr, b1, b2, eps, 0.0)], dtype=torch.float32).to(dev)
    bounds = torch.tensor([0, n], dtype=torch.int64).to(dev)
    out = []
    # whole bucket
    a, b = _state(n, dev, 1), _state(n, dev, 1)
    sa, sb = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
    for _ in range(3):
        engine().call("cc_adam_step", a[0], a[1], a[2], a[3], sa, n, lr, b1, b2, eps, scale, STREAM)
        engine().call("cc_adam_step_hyper", b[0], b[1], b[2], b[3], sb, n, table, bounds, 1, scale, STREAM)
    out += [("whole " + k, x, y) for k, x, y in zip("pgmv", a, b)] + [("whole step", sa, sb)]
    # sub-range: base pointers OFF floats into the allocations; tick on the first call of each step only
    a, b = _state(n, dev, 2, OFF), _state(n, dev, 2, OFF)
    sa, sb = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
    va, vb = [t[OFF:] for t in a], [t[OFF:] for t in b]
    for _ in range(3):
        engine().call("cc_adam_step_segment", va[0], va[1], va[2], va[3], sa, n, lr, b1, b2, eps, scale, 1, STREAM)
        engine().call("cc_adam_step_segment_hyper", vb[0], vb[1], vb[2], vb[3], sb, n, table[0], scale, 1, STREAM)
    out += [("segment " + k, x, y) for k, x, y in zip("pgmv", a, b)] + [("segment step", sa, sb)]      # (the pad in front included)
    _sync(dev)
    assert float(sa) == 3.0 and not torch.equal(a[0], _state(n, dev, 2, OFF)[0])
    return out


BOUNDS = [0, 1088, 2176, 3079]          # boundaries inside 1024-element workgroups; the last row ends in a scalar tail
ROWS = [(1e-4, 0.9, 0.999, 1e-8, 1e-2), (3e-4, 0.8, 0.99, 1e-6, 0.0), (1e-3, 0.95, 0.9, 1e-7, 5e-2)]


def rows_and_bounds(dev, steps=3):
    """Three rows with different hyperparameters over BOUNDS, from zero moments, `steps` steps with a fresh gradient each:
    one whole-bucket launch per step against three sub-range launches per step, and torch.optim.Adam per slice.
    -> (whole [p, m, v], ranges [p, m, v], torch's p)"""
    n, scale = BOUNDS[-1], 0.5
    table = torch.tensor([_row(*r) for r in ROWS], dtype=torch.float32).to(dev)
    bounds = torch.tensor(BOUNDS, dtype=torch.int64).to(dev)
    p0 = _state(n, dev, 3)[0]
    grads = [_state(n, dev, 10 + k)[1] for k in range(steps)]
    w = [p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)]
    r = [p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)]
    sw, sr = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
    ref = [p0[lo:hi].clone().requires_grad_(True) for lo, hi in zip(BOUNDS, BOUNDS[1:])]
    topt = torch.optim.Adam([{"params": [q], "lr": h[0], "betas": (h[1], h[2]), "eps": h[3], "weight_decay": h[4]}
                             for q, h in zip(ref, ROWS)])
    for g in grads:
        engine().call("cc_adam_step_hyper", w[0], g, w[1], w[2], sw, n, table, bounds, len(ROWS), scale, STREAM)
        for k, (lo, hi) in enumerate(zip(BOUNDS, BOUNDS[1:])):
            engine().call("cc_adam_step_segment_hyper", r[0][lo:hi], g[lo:hi], r[1][lo:hi], r[2][lo:hi], sr, hi - lo, table[k],
                          scale, int(k == 0), STREAM)
        for q, (lo, hi) in zip(ref, zip(BOUNDS, BOUNDS[1:])):
            q.grad = g[lo:hi] * scale
        topt.step()
    _sync(dev)
    assert float(sw) == float(sr) == float(steps)
    return w, r, torch.cat([q.detach() for q in ref])


GROUPS = [dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2), dict(lr=3e-4, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.0)]
FACTORS = [1, 1, 10, 10, 0, 5]


def _two_nets():
    return [torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Linear(5, 3)) for _ in range(2)]


def against_torch_adam(dev):
    """Two small networks as two entries of `nets`, GROUPS as their hyperparameters, six steps with both groups' lr multiplied by
    FACTORS through param_groups[..]['lr'] -- FlatAdam, torch.optim.Adam in fp32 and torch.optim.Adam in fp64 on the same problem.
    -> dict(ours, t32, t64: concatenated parameters; zero_step: (p before, p after, exp_avg before, exp_avg after) of the
    factor-0 step of FlatAdam)"""
    torch.manual_seed(0)
    nets = _two_nets()
    init = [n.state_dict() for n in nets]
    x = torch.randn(4, 7)

    def torch_run(dtype):
        ref = _two_nets()
        for n, sd in zip(ref, init):
            n.load_state_dict(sd)
            n.to(device=dev, dtype=dtype)
        topt = torch.optim.Adam([dict(params=list(n.parameters()), **g) for n, g in zip(ref, GROUPS)])
        xx = x.to(device=dev, dtype=dtype)
        for f in FACTORS:
            for g, base in zip(topt.param_groups, GROUPS):
                g["lr"] = base["lr"] * f
            topt.zero_grad()
            sum(n(xx).pow(2).sum() for n in ref).backward()
            topt.step()
        return torch.cat([p.detach().reshape(-1) for n in ref for p in n.parameters()])

    out = {"t32": torch_run(torch.float32), "t64": torch_run(torch.float64)}
    for n in nets:
        n.to(dev)
    opt = T.FlatAdam(nets, T.StepConfig())
    for k, g in enumerate(GROUPS):
        opt.set_hyper(k, **g)
    assert len(opt.param_groups) == 2
    xx = x.to(dev)
    for f in FACTORS:
        for g, base in zip(opt.param_groups, GROUPS):
            g["lr"] = base["lr"] * f
        opt.zero_grad()
        sum(n(xx).pow(2).sum() for n in nets).backward()
        before = (opt.flat_p.clone(), opt.exp_avg.clone())
        opt.step(opt.grad_scale())
        if f == 0:
            out["zero_step"] = (before[0], opt.flat_p.clone(), before[1], opt.exp_avg.clone())
    out["ours"] = opt.gather(opt.flat_p).clone()
    _sync(dev)
    return out
