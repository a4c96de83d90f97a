"""Adam hyperparameters in device memory (cc_adam_step_hyper / cc_adam_step_segment_hyper, FlatAdam's table) on CPU tensors through
the x86 emulation build of the kernel sources; torch.optim.Adam itself is the reference."""
import pytest
import torch

import optim_hyper_cases as C
from cc_amd import trainer as T
from hipemu.emu import emulated_engine


@pytest.mark.parametrize("n", [3 * 1024 + 7, 64])
def test_new_entries_equal_old_entries_bit_for_bit(n):
    """one row, weight decay 0, the same five values: cc_adam_step_hyper == cc_adam_step and cc_adam_step_segment_hyper ==
    cc_adam_step_segment (base pointers 64 floats into the allocations) over three ticks, float4 body and scalar tail"""
    with emulated_engine():
        for name, old, new in C.old_against_new(n, "cpu"):
            assert torch.equal(old, new), name


def test_rows_and_bounds():
    """three rows, bounds inside 1024-element workgroups: one whole-bucket launch == three sub-range launches bit for bit, and every
    range == torch.optim.Adam (weight decay, eps, betas of ITS row) on that slice within 1e-6 absolute"""
    with emulated_engine():
        whole, ranges, want = C.rows_and_bounds("cpu")
    for name, a, b in zip(("p", "exp_avg", "exp_avg_sq"), whole, ranges):
        assert torch.equal(a, b), name
    for lo, hi in zip(C.BOUNDS, C.BOUNDS[1:]):
        d = float((whole[0][lo:hi] - want[lo:hi]).abs().max())
        print("rows [%d, %d): max |FlatAdam kernel - torch.optim.Adam| = %.3e" % (lo, hi, d))
        assert d < 1e-6, (lo, hi, d)


def test_flat_adam_groups_match_torch_adam():
    """two networks = two rows {lr 1e-4, betas (0.9, 0.999), wd 1e-2} / {lr 3e-4, betas (0.8, 0.99), eps 1e-6, wd 0}, six steps under an
    lr schedule written through param_groups: within 1e-6 absolute of torch.optim.Adam (the figure of
    test_flat_adam_matches_torch_adam; torch's own fp32 run stays within the same bound of its fp64 run, which is asserted too).
    The factor-0 step leaves the parameters bit-unchanged while the moments move."""
    with emulated_engine():
        r = C.against_torch_adam("cpu")
    ref_err = float((r["t32"].double() - r["t64"]).abs().max())
    err = float((r["ours"] - r["t32"]).abs().max())
    print("torch fp32 vs torch fp64: %.3e   FlatAdam vs torch fp32: %.3e" % (ref_err, err))
    assert ref_err < 1e-6, ref_err
    assert err < 1e-6, err
    p0, p1, m0, m1 = r["zero_step"]
    assert torch.equal(p0, p1) and not torch.equal(m0, m1)


def _four_nets():
    return [torch.nn.Sequential(torch.nn.Linear(3 + k, 5), torch.nn.Linear(5, 2)) for k in range(4)]


def test_state_dict_and_load_state_dict():
    torch.manual_seed(0)
    with emulated_engine():
        nets = _four_nets()
        opt = T.FlatAdam(nets, T.StepConfig(lr=2e-4, weight_decay=1e-2, eps=1e-7))
        # equal rows: the one-group dictionary, the real eps and weight decay in it
        sd = opt.state_dict()
        assert len(sd["param_groups"]) == 1
        assert sd["param_groups"][0] == {"lr": 2e-4, "betas": (0.9, 0.999), "eps": 1e-7, "weight_decay": 1e-2, "amsgrad": False,
                                         "params": list(range(16))}
        assert opt.lr == 2e-4 and opt.betas == (0.9, 0.999)
        # unequal rows: one group per network, loadable by a torch.optim.Adam built with the same four groups
        opt.set_hyper("pose", lr=5e-5, weight_decay=0.0)
        opt.set_hyper(3, betas=(0.5, 0.9), eps=1e-6)
        assert opt.hyper_of("pose") == {"lr": 5e-5, "betas": (0.9, 0.999), "eps": 1e-7, "weight_decay": 0.0}
        assert opt.hyper_of("disp")["lr"] == 2e-4 and opt.hyper_of("flow")["betas"] == (0.5, 0.9)
        with pytest.raises(ValueError):
            opt.lr
        with pytest.raises(ValueError):
            opt.betas
        opt.zero_grad()
        sum(n(torch.randn(2, 3 + k)).sum() for k, n in enumerate(nets)).backward()
        opt.step()
        sd = opt.state_dict()
        assert [g["params"] for g in sd["param_groups"]] == [list(range(4 * k, 4 * k + 4)) for k in range(4)]
        assert [g["lr"] for g in sd["param_groups"]] == [2e-4, 5e-5, 2e-4, 2e-4]
        tnets = _four_nets()
        topt = torch.optim.Adam([{"params": list(n.parameters())} for n in tnets])
        topt.load_state_dict(sd)
        assert [g["lr"] for g in topt.param_groups] == [2e-4, 5e-5, 2e-4, 2e-4]
        assert topt.param_groups[3]["betas"] == (0.5, 0.9) and topt.param_groups[3]["eps"] == 1e-6
        assert [g["weight_decay"] for g in topt.param_groups] == [1e-2, 0.0, 1e-2, 1e-2]
        p0 = next(tnets[0].parameters())
        assert float(topt.state[p0]["step"]) == 1.0 and topt.state[p0]["exp_avg"].shape == p0.shape
        # round trip through torch's dictionary: table, moments and step counter come back
        opt2 = T.FlatAdam(_four_nets(), T.StepConfig())
        opt2.load_state_dict(topt.state_dict())
        for k in range(4):
            assert opt2.hyper_of(k) == opt.hyper_of(k), k
        assert torch.equal(opt2.exp_avg, opt.exp_avg) and torch.equal(opt2.exp_avg_sq, opt.exp_avg_sq) and float(opt2.step_dev) == 1.0
        opt2.flush_hyper()
        opt.flush_hyper()
        assert torch.equal(opt2.hyper_dev, opt.hyper_dev) and float(opt2.hyper_dev[1, 0]) == pytest.approx(5e-5)
        # one group sets every row (and opt.lr answers again)
        one = T.FlatAdam(_four_nets(), T.StepConfig()).state_dict()
        opt2.load_state_dict(one)
        assert opt2.lr == 1e-4 and opt2.state_dict()["param_groups"][0]["weight_decay"] == 0.0
        # anything that is not one group or the networks' partition in chain order
        moments = (opt2.exp_avg.clone(), float(opt2.step_dev))
        bad = opt.state_dict()
        bad["param_groups"][0]["params"], bad["param_groups"][1]["params"] = list(range(0, 5)), list(range(5, 8))
        two = opt.state_dict()
        two["param_groups"] = [dict(two["param_groups"][0], params=list(range(8))), dict(two["param_groups"][1], params=list(range(8, 16)))]
        short = T.FlatAdam(_four_nets(), T.StepConfig()).state_dict()
        short["param_groups"][0]["params"] = list(range(15))
        for wrong in (bad, two, short):
            with pytest.raises(ValueError):
                opt2.load_state_dict(wrong)
        assert torch.equal(opt2.exp_avg, moments[0]) and float(opt2.step_dev) == moments[1] and opt2.lr == 1e-4     # nothing was taken over


def test_absent_network_keeps_its_row_and_ranges_split_by_row():
    """row index = network index with a network missing; the whole-bucket update, the per-network ranges and a range that spans
    two networks (the legacy pipelines' segments) give the same bits"""
    torch.manual_seed(0)
    with emulated_engine():
        opts = []
        for _ in range(3):
            nets = _four_nets()
            nets[1] = None
            torch.manual_seed(1)
            for n in nets:
                if n is not None:
                    for p in n.parameters():
                        p.data.normal_(0, 0.1)
            opt = T.FlatAdam(nets, T.StepConfig())
            assert len(opt.param_groups) == 3 and [g.net for g in opt.param_groups] == [0, 2, 3]
            assert opt.bounds[1] == opt.bounds[2] == opt.segment(2)[0] and opt.bounds[-1] == opt.flat_p.numel()
            opt.set_hyper("mask", lr=1e-3, weight_decay=0.1)
            opt.set_hyper("flow", lr=0.0)
            opt.param_groups[1]["betas"] = (0.7, 0.9)
            assert opt.hyper_of(2) == {"lr": 1e-3, "betas": (0.7, 0.9), "eps": 1e-8, "weight_decay": 0.1}
            opt.flat_g.copy_(0.05 * torch.randn(opt.flat_g.numel(), generator=torch.Generator().manual_seed(2)))
            opts.append(opt)
        a, b, c = opts
        before = a.flat_p.clone()
        a.step(0.5)
        for k, i in enumerate((0, 2, 3)):
            lo, hi = b.segment(i)
            b.step_segment(lo, hi, k == 0, 0.5)
        c.step_segment(0, c.segment(3)[0], True, 0.5)
        c.step_segment(c.segment(3)[0], None, False, 0.5)
        for o in (b, c):
            assert torch.equal(a.flat_p, o.flat_p) and torch.equal(a.exp_avg, o.exp_avg) and torch.equal(a.exp_avg_sq, o.exp_avg_sq)
            assert float(o.step_dev) == 1.0
        lo, hi = a.segment(3)
        assert torch.equal(a.flat_p[lo:hi], before[lo:hi]) and float(a.exp_avg[lo:hi].abs().max()) > 0        # flow: lr 0
        assert not torch.equal(a.flat_p[:lo], before[:lo])


def test_no_write_while_a_capture_is_in_progress(monkeypatch):
    with emulated_engine():
        opt = T.FlatAdam(_four_nets(), T.StepConfig())
        opt.flush_hyper()
        before = opt.hyper_dev.clone()
        monkeypatch.setattr(T, "_capture_in_progress", lambda t: True)
        with pytest.raises(RuntimeError):
            opt.set_hyper("disp", lr=1.0)
        with pytest.raises(RuntimeError):
            opt.lr = 1.0
        with pytest.raises(RuntimeError):
            opt.param_groups[0]["lr"] = 1.0
        with pytest.raises(RuntimeError):
            opt.load_state_dict(T.FlatAdam(_four_nets(), T.StepConfig(lr=1.0)).state_dict())
        opt.flush_hyper()                   # (declines inside a capture)
        monkeypatch.undo()
        assert opt.lr == 1e-4 and not opt._hyper_dirty
        opt.flush_hyper()
        assert torch.equal(opt.hyper_dev, before)
        opt.lr = 2e-4
        opt.flush_hyper()
        assert float(opt.hyper_dev[0, 0]) == pytest.approx(2e-4) and float(opt.hyper_dev[3, 0]) == pytest.approx(2e-4)


def test_release_moves_the_parameters_out_of_the_buckets(monkeypatch):
    """FlatAdam.release(): same values in storages of their own, no gradients, no sinks, the weight images forgotten -- and the
    modules are as good as new ones: a second FlatAdam over them takes the same first step, bit for bit, as one over a fresh copy
    of the weights"""
    from cc_amd import ops
    torch.manual_seed(0)

    def grad(n, seed):
        return 0.05 * torch.randn(n, generator=torch.Generator().manual_seed(seed))
    with emulated_engine():
        nets = C._two_nets()
        opt = T.FlatAdam(nets, T.StepConfig())
        opt.flat_g.copy_(grad(opt.flat_g.numel(), 2))
        opt.step(0.5)                                   # (the weights are not the initial ones any more)
        params = [p for n in nets for p in n.parameters()]
        want = [p.detach().clone() for p in params]
        resets = []
        monkeypatch.setattr(ops.packs, "reset", lambda: resets.append(1))
        opt.release()
        monkeypatch.undo()
        assert resets == [1]
        for bucket in (opt.flat_p, opt.flat_g):
            lo, hi = bucket.data_ptr(), bucket.data_ptr() + 4 * bucket.numel()
            assert not any(lo <= p.data_ptr() < hi for p in params)
        assert all(torch.equal(p.detach(), w) for p, w in zip(params, want))
        assert all(p.grad is None for p in params) and opt.sinks == {}
        assert len({p.data_ptr() for p in params}) == len(params)
        fresh = C._two_nets()
        for n, m in zip(fresh, nets):
            n.load_state_dict({k: v.clone() for k, v in m.state_dict().items()})
        steps = []
        for mods in (nets, fresh):
            o = T.FlatAdam(mods, T.StepConfig(weight_decay=1e-2))
            o.flat_g.copy_(grad(o.flat_g.numel(), 3))
            o.step(0.5)
            steps.append((o.flat_p, o.exp_avg, o.exp_avg_sq, o.step_dev))
        assert all(torch.equal(a, b) for a, b in zip(*steps))
        assert not torch.equal(steps[0][0], opt.flat_p)       # (the released buckets are nobody's weights any more)
