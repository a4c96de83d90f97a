"""The training driver on the GPU (cc_amd/train.py), each case on trees of its own under tmp_path, at 2 x 64 x 128: the logs against a
hand-written loop over the same public parts, exact resume, fixed networks, the unsupervised validation pass against the oracle,
phases, and the decisive error against the validation passes called directly."""
import os
import random
import types

import numpy as np
import pytest
import torch

import train_cases as C
import validation_store_cases as VC
from cc_amd import custom_transforms as CT
from cc_amd import datasets as DS
from cc_amd import trainer as T
from cc_amd import validate as V

pytestmark = pytest.mark.gpu
DEV = "cuda"
# train.py:34-135's defaults, written out: what the driver must hand to the step when no weight flag is given (the smoothness type
# is the one flag tests/train_cases.py argv() sets)
DEFAULTS = dict(w1=1.0, w2=0.0, w3=0.1, w4=1.0, w5=0.1, wssim=0.0, wrig=1.0, wbce=0.5, THRESH=0.01, qch=0.5, lambda_oob=0.0,
                smoothness_type="edgeaware", lr=2e-4, betas=(0.9, 0.999), weight_decay=0.0)


@pytest.fixture(scope="module")
def straight(tmp_path_factory):
    """run A of two tests: two epochs of two steps straight through, from the seeded weights, no ground truth"""
    tmp = tmp_path_factory.mktemp("straight")
    root = C.data_tree(tmp)
    lines = C.run(C.argv(tmp, root, "a", DEV, "--epochs", "2", "--print-freq", "1"))
    return types.SimpleNamespace(tmp=tmp, root=root, lines=lines, path=C.save_path(tmp, "a"))


def _csv_row(values):
    import csv
    import io
    buf = io.StringIO()
    csv.writer(buf, delimiter='\t').writerow(values)
    return buf.getvalue().strip().split('\t')


def test_logs_equal_a_hand_written_loop(straight):
    full, summary = C.read_tsv(os.path.join(straight.path, "progress_log_full.csv")), C.read_tsv(os.path.join(straight.path, "progress_log_summary.csv"))
    assert full[0] == C.FULL_HEADER and summary[0] == C.SUMMARY_HEADER and len(full) == 5 and len(summary) == 3
    # the same public parts by hand: store, transform, loader, trainer with its ledger -- the same seeds
    store = DS.FrameStore.build(straight.root, train=True, sequence_length=5, device=DEV, workers=2)
    loader = DS.DeviceSequenceLoader(store, C.LB, CT.DeviceTrainTransform(device=DEV, rotate=True, normalize="global"), seed=0)
    assert len(loader) == 2
    tr = T.CCTrainer(C.seeded_nets(DEV), T.StepConfig(ledger=32, **DEFAULTS))
    rows, means = [], []
    for e in range(2):
        random.seed(e)
        np.random.seed(e)
        loader.set_epoch(e)
        for batch in loader:
            tr.step(batch)
        d = tr.ledger.drain()
        assert d.dropped == 0 and d.rows.shape[0] == 2
        rows += [_csv_row([r[1], r[2], 0, r[4], r[5]]) for r in d.rows.tolist()]
        means.append(tr.ledger.average()['loss']['avg'])
        tr.ledger.reset_average()
    assert full[1:] == rows, (full[1:], rows)
    assert [r[0] for r in summary[1:]] == [_csv_row([m])[0] for m in means]
    assert [ln["train_loss"] for ln in straight.lines] == means and [ln["steps"] for ln in straight.lines] == [2, 2]
    assert len({tuple(r) for r in rows}) == 4 and all(0 < float(r[0]) < 1e3 for r in rows)
    # checkpoints: 'epoch' 2 after the second epoch; the best files are the epoch's whose line said is_best
    assert [ln["epoch"] for ln in straight.lines] == [0, 1] and straight.lines[0]["is_best"] is True
    assert all(c["epoch"] == 2 for c in C.load_checkpoints(straight.path))
    best_epoch = 2 if straight.lines[1]["is_best"] else 1
    assert straight.lines[1]["is_best"] == (straight.lines[1]["decisive_error"] <= straight.lines[0]["decisive_error"])
    assert all(c["epoch"] == best_epoch for c in C.load_checkpoints(straight.path, "model_best"))
    assert [float(r[1]) for r in summary[1:]] == [ln["val_loss"] for ln in straight.lines]


def test_resume_is_exact(straight):
    """run B: one epoch, then a second main with --resume up to two epochs in total -- bit for bit run A's five files"""
    from cc_amd import config
    assert config.deterministic
    first = C.run(C.argv(straight.tmp, straight.root, "b", DEV, "--epochs", "1", "--print-freq", "1"))
    assert [ln["epoch"] for ln in first] == [0] and all(c["epoch"] == 1 for c in C.load_checkpoints(C.save_path(straight.tmp, "b")))
    second = C.run(C.argv(straight.tmp, straight.root, "b", DEV, "--epochs", "2", "--print-freq", "1", "--resume"))
    assert [ln["epoch"] for ln in second] == [1]
    a, b = C.load_checkpoints(straight.path), C.load_checkpoints(C.save_path(straight.tmp, "b"))
    n = 0
    for fa, fb in zip(a, b):
        ta, tb = dict(C.tensors_of(fa)), dict(C.tensors_of(fb))
        assert fa["epoch"] == fb["epoch"] == 2 and list(ta) == list(tb)
        for k in ta:
            assert C.same_bits(ta[k], tb[k]), (k, float((ta[k].double() - tb[k].double()).abs().max()))
            n += 1
    assert n > 1000
    assert a[4]["state_dict"]["param_groups"] == b[4]["state_dict"]["param_groups"]
    # the logs were appended to: header, epoch 0, epoch 1 -- the rows of run A
    for name in ("progress_log_full.csv", "progress_log_summary.csv"):
        assert C.read_tsv(os.path.join(C.save_path(straight.tmp, "b"), name)) == C.read_tsv(os.path.join(straight.path, name)), name


def test_fixed_networks_stay_fixed(tmp_path):
    root = C.data_tree(tmp_path)
    C.run(C.argv(tmp_path, root, "fix", DEV, "--epochs", "1", "--fix-masknet", "--fix-flownet"))
    after = C.load_checkpoints(C.save_path(tmp_path, "fix"))
    for k, (name, n) in enumerate(zip(("disp", "pose", "mask", "flow"), C.seeded_nets("cpu"))):
        sd = after[k]["state_dict"]
        same = [C.same_bits(p, sd[key]) for key, p in n.named_parameters()]
        assert len(same) > 0
        if name in ("mask", "flow"):
            assert all(same), name
        else:
            assert not all(same), name
    # the optimizer holds the trained networks' parameters only
    nparams = [len(list(n.parameters())) for n in C.seeded_nets("cpu")]
    assert len(after[4]["state_dict"]["state"]) == nparams[0] + nparams[1]


@pytest.fixture(scope="module")
def oracle_case(tmp_path_factory):
    """the validation samples of the tree as one 2 x 64 x 128 batch on the host and the oracle's six losses for it, computed once"""
    from oracle import step as S
    tmp = tmp_path_factory.mktemp("unsup")
    root = C.data_tree(tmp)
    store = DS.FrameStore.build(root, train=False, sequence_length=5, device=DEV, workers=2)
    assert len(store) == 2 and tuple(store.frames.shape[1:3]) == (C.LH, C.LW)
    x = CT.DeviceFrames(device=DEV).store_to_tensor(store, store.samples_np.T.reshape(-1)).view(5, 2, 3, C.LH, C.LW).cpu()
    K = torch.from_numpy(store.intrinsics_np[store.sample_scene_np])
    batch = (x[0], [x[j] for j in range(1, 5)], K, torch.from_numpy(np.stack([np.linalg.inv(k) for k in K.numpy()])))
    onets = S.build_nets("oracle")
    for n in onets:
        n.load_state_dict(C.syn.seeded_state_dict(n, 0))
        n.eval()
    with torch.no_grad():
        # the eval-mode outputs are one full-resolution level each: the restated train.py:454-509 over one-level lists
        as_levels = (lambda t: [onets[0](t)], onets[1], lambda t, r: [onets[2](t, r)],
                     lambda t, r: tuple([v] for v in onets[3](t, r)))
        want = S.cc_forward(as_levels, batch, S.StepConfig())
    return types.SimpleNamespace(root=root, store=store, want={k: float(v) for k, v in want.items() if k.startswith("loss")})


def test_unsupervised_pass_against_oracle(oracle_case):
    nets = C.seeded_nets(DEV)
    got, names = V.validate_without_gt_from_store(oracle_case.store, *nets, 2, T.StepConfig())
    assert names == ["loss", "loss_1", "loss_2", "loss_3", "loss_4", "loss_5"] and all(not n.training for n in nets)
    for k, g in zip(names, got):
        w = oracle_case.want[k]
        print("unsupervised %-7s hip %.8f  oracle %.8f  rel %.2e" % (k, g, w, abs(g - w) / abs(w)))
    for k, g in zip(names, got):
        w = oracle_case.want[k]
        assert w != 0 and abs(g - w) <= 1e-4 * abs(w), (k, g, w)


def test_unsupervised_pass_batch_sizes_agree(oracle_case):
    """four samples (of the training list: two scenes), batch sizes 1 and 2: the same six means"""
    full = DS.FrameStore.build(oracle_case.root, train=True, sequence_length=5, device=DEV, workers=2)
    four = DS.FrameStore(full.frames, full.minmax, full.intrinsics, full.samples[1:5], full.sample_scene[1:5], full.scenes)
    assert len(four) == 4 and len(set(four.sample_scene.tolist())) == 2
    nets = C.seeded_nets(DEV)
    cfg = T.StepConfig()
    one, _ = V.validate_without_gt_from_store(four, *nets, 1, cfg)
    two, _ = V.validate_without_gt_from_store(four, *nets, 2, cfg)
    three, _ = V.validate_without_gt_from_store(four, *nets, 3, cfg)          # a short last batch weighs by its size
    for a, b, c in zip(one, two, three):
        assert a != 0 and abs(a - b) <= 1e-4 * abs(a) and abs(a - c) <= 1e-4 * abs(a), (one, two, three)


def test_phases(tmp_path, monkeypatch):
    """--phases "disp+pose:1,flow:1" --cycles 3 at two steps per epoch: a trainer per phase, only the phase's networks change, six
    epochs are written, and torch.cuda.memory_allocated() after cycle 3 is not above its value after cycle 2 (what a dropped
    trainer used to leave behind -- BLAS workspaces, the network contexts of its captured step -- is in NOTES.md)"""
    root = C.data_tree(tmp_path)
    seen = []
    orig = T.CCTrainer.save_checkpoint

    def spy(self, save_path, epoch, is_best=False):
        seen.append((epoch, torch.cuda.memory_allocated(), [[p.detach().cpu().clone() for p in n.parameters()] for n in self.nets]))
        return orig(self, save_path, epoch, is_best)
    monkeypatch.setattr(T.CCTrainer, "save_checkpoint", spy)
    built, make = [], C.TR.make_trainer
    monkeypatch.setattr(C.TR, "make_trainer", lambda args, nets, trained, dev: built.append(trained) or make(args, nets, trained, dev))
    lines = C.run(C.argv(tmp_path, root, "ph", DEV, "--phases", "disp+pose:1,flow:1", "--cycles", "3", "--fix-dispnet", "--epochs", "50"))
    assert [ln["epoch"] for ln in lines] == list(range(6)) == [s[0] for s in seen] and all(ln["steps"] == 2 for ln in lines)
    assert [ln["phase"] for ln in lines] == ["disp+pose", "flow"] * 3 and [ln["cycle"] for ln in lines] == [0, 0, 1, 1, 2, 2]
    assert built == [("disp", "pose"), ("flow",)] * 3                         # a trainer per phase
    assert all(ln["is_best"] for ln in lines[:2])                             # the best error is kept per set: each set's first epoch
    prev = [list(n.parameters()) for n in C.seeded_nets("cpu")]
    for e, (_, _, params) in enumerate(seen):
        trained = {"disp", "pose"} if e % 2 == 0 else {"flow"}
        for name, before, after in zip(("disp", "pose", "mask", "flow"), prev, params):
            same = [C.same_bits(a, b) for a, b in zip(before, after)]
            assert (not all(same)) if name in trained else all(same), (e, name)
        prev = params
    assert seen[5][1] <= seen[3][1], [s[1] for s in seen]                      # device memory after cycle 3 against after cycle 2
    assert all(c["epoch"] == 6 for c in C.load_checkpoints(C.save_path(tmp_path, "ph")))
    assert len(C.read_tsv(os.path.join(C.save_path(tmp_path, "ph"), "progress_log_summary.csv"))) == 7


def test_decisive_error_is_the_validation_pass_entry(tmp_path):
    """both tiny ground-truth stores: pose trained -> flow_errors[-2]; pose fixed, disp trained -> errors[0] (train.py:382-385)"""
    root = C.data_tree(tmp_path, "cityscapes_t")
    val_root = VC.build_val_tree(tmp_path / "kitti_t", C.LH, C.LW)           # train.py:205: 'cityscapes' -> 'kitti'
    VC.make_flow_tree(tmp_path / "kitti2015", VC.FLOW_SIZES)
    gt = ["--with-depth-gt", "--with-flow-gt", "--kitti-dir", str(tmp_path / "kitti2015"), "--flow-size", "64", "192", "--val-batch-size", "2",
          "--epochs", "1", "--epoch-size", "1"]
    from cc_amd import kitti_eval as K
    flow_store = DS.FlowValStore.build(K.Kitti2015Flow(tmp_path / "kitti2015", N=len(VC.FLOW_SIZES)), (64, 192), device=DEV)
    depth_store = DS.DepthValStore.build(val_root, device=DEV, workers=2)
    args = types.SimpleNamespace(THRESH=0.01, flownet="Back2Future", spatial_normalize=False)
    for name, extra, pick in (("dp", [], "flow"), ("dd", ["--fix-posenet"], "depth")):
        lines = C.run(C.argv(tmp_path, root, name, DEV, *(gt + extra)))
        summary = C.read_tsv(os.path.join(C.save_path(tmp_path, name), "progress_log_summary.csv"))
        nets = T.build_nets(DEV, init=False)
        for n, c in zip(nets, C.load_checkpoints(C.save_path(tmp_path, name))):
            n.load_state_dict(c["state_dict"])
        if pick == "flow":
            errors, names = V.validate_flow_from_store(flow_store, *nets, batch_size=2, args=args)
            want, dname = errors[-2], names[-2]
        else:
            errors, names = V.validate_depth_from_store(depth_store, nets[0], 2, args=args)
            want, dname = errors[0], names[0]
        assert np.isfinite(want) and float(summary[1][1]) == want == lines[0]["decisive_error"], (name, summary[1], want)
        assert lines[0]["decisive"] == dname and "val_loss" not in lines[0]                     # no train=False store was needed
        assert lines[0]["abs_diff"] > 0 and lines[0]["epe_total"] > 0
