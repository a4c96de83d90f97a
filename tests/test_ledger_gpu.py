"""The step ledger and the per-parameter statistics on the MI355X: the kernels' cases of tests/ledger_cases.py on the product
library, the ledger's append as the last node of a captured step (and as the last call of an eager and of a legacy-form step), and
FlatAdam.param_stats() on the buckets of a real step."""
import collections
import math

import pytest
import torch

import grad_guard_cases as G
import ledger_cases as C
from cc_amd import config, synthetic as syn, trainer as T

pytestmark = pytest.mark.gpu

DEV = "cuda"
POSE_LR = 3e-4


@pytest.mark.parametrize("guard", [False, True])
def test_rows_and_aggregates_on_device(guard):
    C.check_rows_and_aggregates(DEV, guard)


def test_resets_and_resume_on_device():
    C.check_resets(DEV)


def test_non_finite_values_on_device():
    C.check_nonfinite(DEV)


def test_log_file_on_device(tmp_path):
    C.check_log_file(DEV, tmp_path)


def test_ledger_reads_flat_adams_tables_on_device():
    C.check_ledger_follows_flat_adam(DEV)


def test_param_stats_synthetic_bucket_on_device():
    C.check_param_stats(DEV)


def test_param_stats_non_finite_placement_on_device():
    C.check_param_stats_nonfinite(DEV)


# ------------------------------------------------------------------------------------------------------------ in the step
def _batch(dev):
    bc = syn.sample(2, 128, 192, seed=1)
    return (bc[0].to(dev), [r.to(dev) for r in bc[1]], bc[2].to(dev), bc[3].to(dev))


def _trainer(cfg, **kw):
    dev = torch.device("cuda")
    nets = T.build_nets(dev, init=False)
    for n in nets:
        n.load_state_dict(syn.seeded_state_dict(n, 0))
    return T.CCTrainer(nets, cfg, **kw)


def _three_steps(tr, batch):
    """three steps, PoseNetB6's lr changed between the second and the third; the losses and the guard rows are read back after
    every step (this test only: it is what the ledger saves a training loop from)
    -> per step {"losses": {name: 1-element fp32 CPU tensor}, "stats": grad_stats(sync=True)}, the graph objects seen"""
    out, graphs = [], []
    for s in range(3):
        if s == 2:
            tr.opt.set_hyper("pose", lr=POSE_LR)
        losses = tr.step(batch)
        torch.cuda.synchronize()
        out.append({"losses": {k: v.detach().reshape(1).cpu().clone() for k, v in losses.items()}, "stats": tr.grad_stats(sync=True)})
        graphs.append(tr.graph)
    return out, graphs


def _state(tr):
    torch.cuda.synchronize()
    return {"p": tr.opt.flat_p.clone(), "m": tr.opt.exp_avg.clone(), "v": tr.opt.exp_avg_sq.clone(), "g": tr.opt.flat_g.clone(),
            "step": float(tr.opt.step_dev)}


def _warm_up_like_capture(tr, batch):
    """What capture() does for a captured trainer, for an eager one: one throw-away eager step, then parameters, moments, counter,
    guard rows, BatchNorm buffers and the ledger are put back.  A trainer's very first step finds no weight images registered
    (ops.packs), so the grouped data-gradient calls of that one step take the per-layer path with another split of the reduction
    (conv.hip dgrad_group_impl): Back2Future's gradient differs from every later step's in the last bits (about 1e-9 absolute; the
    emulation build shows it too).  Every step of a captured trainer runs behind capture()'s warm-up; "the same three steps" of the
    eager trainer are compared from the same footing."""
    opt = tr.opt
    keep = [(t, t.detach().clone()) for t in (opt.flat_p, opt.exp_avg, opt.exp_avg_sq, opt.step_dev, opt.guard_dev, tr.ledger.state)] + \
           [(b, b.detach().clone()) for n in tr.nets for b in n.buffers()]
    tr.step(batch)
    torch.cuda.synchronize()
    for t, saved in keep:
        t.copy_(saved)              # (flat_p's version counter moves: the next step rebuilds every weight image, as capture() does)


@pytest.fixture(scope="module")
def runs():
    """Guard on without clipping (max_grad_norm = inf) everywhere.  A: ledger off, captured; B: ledger on, captured; C: ledger on,
    eager; D: ledger on, pipeline 'post'.  One after the other: ops.packs belongs to the trainer built last."""
    batch = _batch(torch.device("cuda"))
    old = config.deterministic
    config.deterministic = True
    out = {}
    try:
        a = _trainer(T.StepConfig(max_grad_norm=G.INF), use_graph=True)
        assert a.pipeline == "per_network" and a.ledger is None
        with G.CallLog() as calls:
            out["steps_a"], _ = _three_steps(a, batch)
        out["calls_a"], out["state_a"] = collections.Counter(calls.names), _state(a)
        del a

        b = _trainer(T.StepConfig(max_grad_norm=G.INF, ledger=8), use_graph=True)
        with G.CallLog() as calls:
            out["steps_b"], graphs = _three_steps(b, batch)
        out["calls_b"], out["state_b"] = collections.Counter(calls.names), _state(b)
        out["same_graph"] = graphs[0] is not None and all(g is graphs[0] for g in graphs)
        out["head_b"] = int(b.ledger.head)
        # parameter statistics of the third step's gradient, and what they leave alone
        before = [t.clone() for t in (b.opt.flat_p, b.opt.flat_g, b.opt.exp_avg, b.opt.exp_avg_sq, b.ledger.state)]
        views = b.param_stats()
        out["pstats"] = b.param_stats(sync=True)
        out["first_nonfinite"] = b.first_nonfinite()
        torch.cuda.synchronize()
        out["untouched"] = all(torch.equal(x, y) for x, y in zip(before, (b.opt.flat_p, b.opt.flat_g, b.opt.exp_avg, b.opt.exp_avg_sq,
                                                                          b.ledger.state)))
        v = next(iter(views.values()))["grad_norm"]
        out["views_ok"] = torch.is_tensor(v) and v.is_cuda and v.dim() == 0 and list(views) == b.opt.param_names
        out["net_of"] = {name: name.split(".")[0] for name in b.opt.param_names}
        out["drain_b"], out["absent_b"] = b.ledger.drain(), set(b.ledger.absent)
        out["avg_b"] = b.ledger.average()
        # a re-capture keeps the ledger and its head
        led = b.ledger
        b.switch_pipeline("per_network")
        b.step(batch)
        torch.cuda.synchronize()
        out["recapture"] = (b.ledger is led, b.graph is not graphs[0], int(led.head), led.drain())
        del b

        c = _trainer(T.StepConfig(max_grad_norm=G.INF, ledger=8), use_graph=False)
        assert c.pipeline == "per_network"
        _warm_up_like_capture(c, batch)
        out["head_c0"] = int(c.ledger.head)
        out["steps_c"], _ = _three_steps(c, batch)
        out["drain_c"] = c.ledger.drain()
        del c

        d = _trainer(T.StepConfig(max_grad_norm=G.INF, ledger=8), use_graph=True, pipeline="post")
        assert d.pipeline == "post"
        out["steps_d"], _ = _three_steps(d, batch)
        out["drain_d"], out["head_d"] = d.ledger.drain(), int(d.ledger.head)
        del d
    finally:
        config.deterministic = old
    return out


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check_rows(rows, steps):
    """every row against what was read back after its step"""
    assert tuple(rows.shape) == (3, 32)
    assert rows[:, 0].tolist() == [1.0, 2.0, 3.0]
    for k, st in enumerate(steps):
        want = torch.cat([st["losses"][name] for name in C.NAMES])
        assert torch.equal(_bits(rows[k, 1:7]), _bits(want)), (k, rows[k, 1:7], want)
        assert float(rows[k, 7]) == 0.0
        lr = [1e-4, POSE_LR if k == 2 else 1e-4, 1e-4, 1e-4]
        assert rows[k, 8:12].tolist() == torch.tensor(lr, dtype=torch.float32).tolist(), (k, rows[k, 8:12])
        assert rows[k, 12:16].tolist() == [st["stats"][n]["norm"] for n in T.NET_NAMES], k
        assert rows[k, 16:20].tolist() == [1.0] * 4 and rows[k, 20:24].tolist() == [1.0] * 4
        assert float(rows[k, 24:].abs().max()) == 0.0


def test_ledger_on_changes_nothing_but_its_own_launch(runs):
    for sa, sb in zip(runs["steps_a"], runs["steps_b"]):
        for k in sa["losses"]:
            assert torch.equal(_bits(sa["losses"][k]), _bits(sb["losses"][k])), k
        assert sa["stats"] == sb["stats"]
    a, b = runs["state_a"], runs["state_b"]
    assert a["step"] == b["step"] == 3.0
    for k in ("p", "m", "v"):
        assert torch.equal(a[k], b[k]), (k, float((a[k] - b[k]).abs().max()))
    ca, cb = dict(runs["calls_a"]), dict(runs["calls_b"])
    assert not any(k.startswith("cc_ledger") for k in ca)
    # capture = two eager warm-up steps + the captured one: three calls of the entry; the replays make none
    assert cb.pop("cc_ledger_append") == 3 and not any(k.startswith("cc_ledger") for k in cb)
    # cc_conv2d_wgrad_ws_bytes is no launch: a host-side size query that ops._wgrad_ws_bytes memoises per process and geometry, so
    # the trainer built second can only ask it less often than the one built first.  Every other entry: the same count.
    memo = "cc_conv2d_wgrad_ws_bytes"
    assert cb.pop(memo, 0) <= ca.pop(memo, 0)
    assert ca == cb


def test_rows_of_the_captured_step(runs):
    assert runs["head_b"] == 3, "the warm-up steps of capture() left rows behind"
    assert runs["same_graph"], "set_hyper made the trainer capture again"
    d = runs["drain_b"]
    assert d.first_iter == 0 and d.dropped == 0 and runs["absent_b"] == set()
    _check_rows(d.rows, runs["steps_b"])
    want = sum(2.0 * float(s["losses"]["loss"].double()) for s in runs["steps_b"]) / 6.0
    got = runs["avg_b"]["loss"]
    assert got["weight"] == 6.0 and abs(got["avg"] - want) <= 1e-15 * abs(want), (got, want)
    same_ledger, new_graph, head, again = runs["recapture"]
    assert same_ledger and new_graph and head == 4 and again.first_iter == 3 and again.rows[:, 0].tolist() == [4.0]


def test_rows_of_eager_steps(runs):
    """use_graph=False: every row is the eager step's own losses, counter, learning rates and guard rows, and the three rows are
    bit for bit the captured trainer's (both behind one warm-up, see _warm_up_like_capture)"""
    d = runs["drain_c"]
    assert runs["head_c0"] == 0 and d.first_iter == 0 and d.dropped == 0
    _check_rows(d.rows, runs["steps_c"])
    b, c = runs["drain_b"].rows, d.rows
    diff = float((b.double() - c.double()).abs().max())
    print("captured vs eager rows: max |difference| = %.3e" % diff)
    assert torch.equal(_bits(b), _bits(c)), diff


def test_legacy_form_appends_one_row_per_step(runs):
    d = runs["drain_d"]
    assert runs["head_d"] == 3 and d.first_iter == 0 and d.dropped == 0
    _check_rows(d.rows, runs["steps_d"])


def test_param_stats_of_a_real_step(runs):
    assert runs["views_ok"] and runs["untouched"] and runs["first_nonfinite"] is None
    stats = runs["steps_b"][2]["stats"]
    sq = collections.defaultdict(float)
    for name, st in runs["pstats"].items():
        sq[runs["net_of"][name]] += st["grad_norm"] ** 2
        assert st["nonfinite"] == 0.0 and st["weight_norm"] >= 0.0 and 0.0 <= st["grad_maxabs"] <= st["grad_norm"] * (1 + 1e-12)
    assert set(sq) == set(T.NET_NAMES)
    for net in T.NET_NAMES:
        got, want = math.sqrt(sq[net]), stats[net]["norm"]
        rel = abs(got - want) / want
        print("%s: sqrt(sum of per-parameter grad_norm^2) %.9g, guard norm %.9g, rel %.2e" % (net, got, want, rel))
        assert rel < 1e-6, (net, got, want)


def test_first_nonfinite_names_the_network_the_inf_reached():
    """the guard test's scenario (w4 = inf: Back2Future's gradient, and MaskNet6's through 1 - m[:, 1:3], is not finite; DispResNet6
    and PoseNetB6 get theirs from l1 / l3 / l5), two steps"""
    batch = _batch(torch.device("cuda"))
    old = config.deterministic
    config.deterministic = True
    try:
        c = _trainer(T.StepConfig(w4=G.INF, max_grad_norm=G.INF), use_graph=True)
        c.step(batch)
        c.step(batch)
        name = c.first_nonfinite()
        st = c.param_stats(sync=True)
        del c
    finally:
        config.deterministic = old
    assert name is not None and name.split(".")[0] in ("mask", "flow"), name
    assert st[name]["nonfinite"] > 0
    assert all(v["nonfinite"] == 0.0 for k, v in st.items() if k.split(".")[0] in ("disp", "pose"))
    assert name == next(k for k, v in st.items() if v["nonfinite"] > 0)
