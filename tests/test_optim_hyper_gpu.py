"""Adam hyperparameters in device memory on the MI355X: the table-driven kernel against the old entries and torch.optim.Adam, and a
change of lr / of one network's row reaching a step that was captured into a hipGraph before the change."""
import pytest
import torch

import optim_hyper_cases as C
from cc_amd import config, synthetic as syn, trainer as T, utils

pytestmark = pytest.mark.gpu

NEW_LR = 2.5e-5


@pytest.mark.parametrize("n", [3 * 1024 + 7, 64])
def test_new_entries_equal_old_entries_bit_for_bit_on_device(n):
    for name, old, new in C.old_against_new(n, "cuda"):
        assert torch.equal(old, new), name


def test_rows_and_bounds_on_device():
    whole, ranges, want = C.rows_and_bounds("cuda")
    for name, a, b in zip(("p", "exp_avg", "exp_avg_sq"), whole, ranges):
        assert torch.equal(a, b), name
    for lo, hi in zip(C.BOUNDS, C.BOUNDS[1:]):
        d = float((whole[0][lo:hi] - want[lo:hi]).abs().max())
        print("rows [%d, %d): max |FlatAdam kernel - torch.optim.Adam| = %.3e" % (lo, hi, d))
        assert d < 1e-6, (lo, hi, d)


def test_weight_decay_and_groups_match_torch_adam_on_device():
    """tests/test_optim_hyper.py::test_flat_adam_groups_match_torch_adam with every tensor on the GPU, torch's own Adam (fp32, and
    fp64 as its yardstick) as the reference, the same 1e-6 absolute bound"""
    r = C.against_torch_adam("cuda")
    ref_err = float((r["t32"].double() - r["t64"]).abs().max())
    err = float((r["ours"] - r["t32"]).abs().max())
    print("torch fp32 vs torch fp64: %.3e   FlatAdam vs torch fp32: %.3e" % (ref_err, err))
    assert ref_err < 1e-6, ref_err
    assert err < 1e-6, err
    p0, p1, m0, m1 = r["zero_step"]
    assert torch.equal(p0, p1) and not torch.equal(m0, m1)


def _batch(dev):
    bc = syn.sample(2, 128, 192, seed=1)
    return (bc[0].to(dev), [r.to(dev) for r in bc[1]], bc[2].to(dev), bc[3].to(dev))


def _snapshot(tr, losses):
    torch.cuda.synchronize()
    return {"p": tr.opt.flat_p.clone(), "m": tr.opt.exp_avg.clone(), "v": tr.opt.exp_avg_sq.clone(),
            "losses": {k: float(x) for k, x in losses.items()}}


def _change_after_capture(pipeline, path, hold=None):
    """Trainer A: two steps (the second a replay of the captured step), checkpoint, lr -> NEW_LR, step 3 -- and, with `hold`, a
    fourth step with that network's lr at 0.  Trainer B: fresh from the checkpoint with lr = NEW_LR BEFORE its first step (the
    value is right at capture time), step 3.  A takes all its steps before B is built: the weight-image registry (ops.packs) is
    one per process and belongs to the trainer built last.
    -> (A, A's graph before the change, A after step 3, B after step 3, (p, exp_avg before step 4, p, exp_avg after) or None)"""
    dev = torch.device("cuda")
    batch = _batch(dev)
    old = config.deterministic
    config.deterministic = True
    try:
        nets = T.build_nets(dev, init=False)
        for n in nets:
            n.load_state_dict(syn.seeded_state_dict(n, 0))
        a = T.CCTrainer(nets, T.StepConfig(), use_graph=True, pipeline=pipeline)
        assert a.pipeline == pipeline
        a.step(batch)
        a.step(batch)
        torch.cuda.synchronize()
        a.save_checkpoint(path, epoch=0, is_best=False)
        g0 = a.graph
        assert g0 is not None
        a.opt.lr = NEW_LR
        sa = _snapshot(a, a.step(batch))
        held = None
        if hold is not None:
            before = (sa["p"], sa["m"])
            a.opt.set_hyper(hold, lr=0.0)
            assert a.opt.hyper_of(hold)["lr"] == 0.0 and all(a.opt.hyper_of(n)["lr"] == NEW_LR for n in T.NET_NAMES if n != hold)
            a.step(batch)
            torch.cuda.synchronize()
            held = before + (a.opt.flat_p.clone(), a.opt.exp_avg.clone())
        g1 = a.graph
        nets2 = T.build_nets(dev, init=True)
        assert utils.resume(path, *nets2, map_location=dev) == 1
        b = T.CCTrainer(nets2, T.StepConfig(), use_graph=True, pipeline=pipeline)
        assert utils.resume_optimizer(path, b, map_location=dev) is True
        b.opt.lr = NEW_LR
        assert float(b.opt.step_dev) == 2.0
        sb = _snapshot(b, b.step(batch))
        del b
    finally:
        config.deterministic = old
    assert g1 is g0, "the step was captured again"
    return a, g0, sa, sb, held


def _assert_same_step(sa, sb):
    assert sa["losses"] == sb["losses"], (sa["losses"], sb["losses"])
    for k in ("p", "m", "v"):
        assert torch.equal(sa[k], sb[k]), (k, float((sa[k] - sb[k]).abs().max()))


@pytest.fixture(scope="module")
def captured(tmp_path_factory):
    return _change_after_capture("per_network", tmp_path_factory.mktemp("ckpt"), hold="pose")


def test_lr_change_reaches_the_captured_step(captured):
    """default pipeline: the Adam launches are nodes of the captured graph -- `tr.opt.lr = x` after the capture must hold for the next
    replay, bit for bit the step of a trainer that was captured with x, and the graph is the one captured before"""
    a, g0, sa, sb, _ = captured
    assert a.pipeline == "per_network"
    _assert_same_step(sa, sb)
    assert a.graph is g0


def test_one_network_held_still_on_the_captured_step(captured):
    """set_hyper('pose', lr=0) on the captured trainer, one more step: PoseNetB6's segment of the parameters stays bit for bit while
    its moments go on, the other three networks move, no graph is captured again"""
    a, g0, _, _, (p0, m0, p1, m1) = captured
    for i, name in enumerate(T.NET_NAMES):
        lo, hi = a.opt.segment(i)
        if name == "pose":
            assert torch.equal(p1[lo:hi], p0[lo:hi]) and not torch.equal(m1[lo:hi], m0[lo:hi])
        else:
            assert not torch.equal(p1[lo:hi], p0[lo:hi]), name
    assert a.graph is g0


@pytest.mark.parametrize("pipeline", ["post", "staged"])
def test_lr_change_reaches_the_other_pipelines(pipeline, tmp_path):
    a, g0, sa, sb, _ = _change_after_capture(pipeline, tmp_path)
    _assert_same_step(sa, sb)
    assert a.graph is g0
