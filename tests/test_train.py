"""The training driver on the host (cc_amd/train.py): its flags against the reference's (tests/golden/train_args.json, written by
tools/make_train_golden.py from the unmodified train.py:34-135), the refusals, the phase syntax, the decisive-error table of
train.py:382-389, and -- on the x86 emulation build, slow -- one epoch end to end."""
import itertools
import json
import os

import pytest

import frame_store_cases as FC
from cc_amd import train as TR
from cc_amd import validate as V

# the deviation table of cc_amd/train.py, as far as it touches the flags: dest -> (field, the driver's value)
DEVIATIONS = {"posenet": ("default", "PoseNetB6"), "masknet": ("default", "MaskNet6"), "flownet": ("default", "Back2Future")}
DRIVER_ONLY = {"phases": None, "cycles": 1, "val_batch_size": 8, "flow_size": [256, 832], "store_cache": None, "max_grad_norm": None,
               "checkpoint_root": "checkpoints", "device": "cuda"}


def _describe(action):
    kind = {"_StoreAction": "store", "_StoreTrueAction": "store_true"}[type(action).__name__]
    return {"strings": list(action.option_strings) or [action.dest], "dest": action.dest,
            "type": action.type.__name__ if action.type is not None else None, "default": action.default,
            "choices": list(action.choices) if action.choices is not None else None, "action": kind, "required": bool(action.required)}


def test_parser_matches_reference_flags(golden_dir):
    with open(os.path.join(golden_dir, "train_args.json")) as f:
        gold = json.load(f)
    assert len(gold) == 60
    p = TR.build_parser()
    mine = {a.dest: _describe(a) for a in p._actions if a.dest != "help"}
    seen = set()
    for g in gold:
        m = mine[g["dest"]]
        seen.add(g["dest"])
        for field in ("strings", "dest", "type", "default", "choices", "action", "required"):
            if g["strings"] == ["data"] and field == "required":
                continue                                            # (a positional: argparse marks it required itself)
            if DEVIATIONS.get(g["dest"], (None,))[0] == field:
                assert m[field] == DEVIATIONS[g["dest"]][1] and m[field] != g[field], (g["dest"], field)
                continue
            assert m[field] == g[field] and type(m[field]) is type(g[field]), (g["dest"], field, m[field], g[field])
    name = [g for g in gold if g["dest"] == "name"][0]
    assert name["required"] is True and mine["name"]["required"] is True
    # the reference's three defaults name no module of models; the driver's do
    from cc_amd import models
    for dest in DEVIATIONS:
        g = [x for x in gold if x["dest"] == dest][0]
        assert not hasattr(models, g["default"]) and hasattr(models, mine[dest]["default"]) and mine[dest]["default"] in g["choices"]
    assert set(mine) - seen == set(DRIVER_ONLY)
    args = p.parse_args(["D", "--name", "n"])
    for dest, default in DRIVER_ONLY.items():
        assert getattr(args, dest) == default, dest
    assert p.parse_args(["D", "--name", "n", "--flow-size", "64", "192"]).flow_size == [64, 192]
    with pytest.raises(SystemExit):
        p.parse_args(["D"])                                         # --name is required


REFUSALS = [
    (["--robust"], "photometric_reconstruction_loss_robust"),
    (["--joint-mask-for-depth"], "compute_joint_mask_for_depth"),
    (["--dataset-format", "stacked"], "sequence folders only"),
    (["--sequence-length", "3"], "ref_imgs[1:3]"),
    (["--fix-dispnet", "--fix-posenet", "--fix-masknet", "--fix-flownet"], "nothing to train"),
    (["--flownet", "FlowNetC6"], "Back2Future's joint"),
    (["--flow-size", "250", "832"], "multiples of 64"),
    (["--cycles", "2"], "--cycles needs --phases"),
    (["--phases", "disp+depth:3"], "unknown network 'depth'"),
]


@pytest.mark.parametrize("extra,message", REFUSALS, ids=[" ".join(e) for e, _ in REFUSALS])
def test_refusals_say_why(extra, message, capsys):
    with pytest.raises(SystemExit) as e:
        TR.main(["/nowhere", "--name", "n"] + extra)
    assert e.value.code == 2 and message in capsys.readouterr().err


def test_refuses_more_than_one_process(monkeypatch, capsys):
    """WORLD_SIZE > 1 is refused: given by the caller, read off an initialised process group, or implied by torchrun (the package
    itself reads no environment variable, tests/test_abi.py)"""
    import torch.distributed as dist
    with pytest.raises(SystemExit):
        TR.main(["/nowhere", "--name", "n"], world_size=2)
    assert "world_size = 2: this driver is one process on one GPU" in capsys.readouterr().err
    monkeypatch.setenv("TORCHELASTIC_RUN_ID", "job0")
    with pytest.raises(SystemExit):
        TR.main(["/nowhere", "--name", "n"])
    assert "started by torchrun: this driver is one process on one GPU" in capsys.readouterr().err
    monkeypatch.delenv("TORCHELASTIC_RUN_ID")
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda: 4)
    assert TR.launched_world_size() == (4, "a process group of 4 ranks is initialised")
    monkeypatch.undo()
    assert TR.launched_world_size() == (1, "") and TR.launched_world_size(1)[0] == 1


def test_refuses_frames_that_are_no_multiple_of_64(tmp_path, capsys):
    root = FC.build_tree(tmp_path / "tree", 40, 128)
    with pytest.raises(SystemExit):
        TR.main([root, "--name", "n", "--checkpoint-root", str(tmp_path / "ck")])
    assert "frames of 40 x 128" in capsys.readouterr().err and not (tmp_path / "ck").exists()
    root = FC.build_tree(tmp_path / "tree2", 64, 96)
    with pytest.raises(SystemExit):
        TR.main([root, "--name", "n", "--checkpoint-root", str(tmp_path / "ck")])
    assert "frames of 64 x 96" in capsys.readouterr().err


def test_no_effect_flags_parse():
    args = TR.build_parser().parse_args(["D", "--name", "n", "-f", "5", "--log-output", "--log-terminal", "--alternating", "--clamp-masks",
                                         "--fix-posemasknet", "-e"])
    assert all(getattr(args, dest) for dest, _ in TR.NO_EFFECT) and len(TR.NO_EFFECT) == 7


def test_phase_strings():
    assert TR.parse_phases("disp+pose:30,flow:30,mask:10") == [(("disp", "pose"), 30), (("flow",), 30), (("mask",), 10)]
    assert TR.parse_phases(" pose+disp:1 , flow+mask+disp:2") == [(("disp", "pose"), 1), (("disp", "mask", "flow"), 2)]     # chain order
    for bad, why in (("disp", "NETS:EPOCHS"), ("disp:", "NETS:EPOCHS"), (":3", "NETS:EPOCHS"), ("disp:0", "0 epochs"), ("disp:-1", "-1 epochs"),
                     ("disp:x", "'x' epochs"), ("disp+disp:2", "named twice"), ("depth:2", "unknown network 'depth'"), ("disp:1,,flow:1", "NETS:EPOCHS"),
                     ("disp+:1", "unknown network ''"), ("", "NETS:EPOCHS")):
        with pytest.raises(ValueError, match=why):
            TR.parse_phases(bad)
    p = TR.build_parser()
    a = p.parse_args(["D", "--name", "n", "--phases", "disp+pose:2,flow:1", "--cycles", "3", "--fix-dispnet", "--epochs", "7"])
    plan = TR.schedule(a)                                            # overrides --fix-* and --epochs; the epoch counter runs on
    assert plan == [(c, names, 3 * c + lo, 3 * c + hi) for c in range(3) for names, lo, hi in ((("disp", "pose"), 0, 2), (("flow",), 2, 3))]
    a = p.parse_args(["D", "--name", "n", "--fix-masknet", "--fix-flownet", "--epochs", "7"])
    assert TR.schedule(a) == [(0, ("disp", "pose"), 0, 7)]


def _reference_choice(fix):
    """train.py:382-389, restated"""
    if not fix["pose"]:
        return "flow", -2
    if not fix["disp"]:
        return "depth", 0
    if not fix["flow"]:
        return "flow", -1
    if not fix["mask"]:
        return "flow", 3


def test_decisive_error_table():
    # the indices are the reference's; the names beside them in train.py:383,387 are one off (its list has eight entries, :641)
    assert V.FLOW_ERROR_NAMES[-2] == "epe_non_rigid_with_gt_mask" and V.FLOW_ERROR_NAMES[-1] == "outliers_gt_mask" and \
        V.FLOW_ERROR_NAMES[3] == "outliers" and V.DEPTH_ERROR_NAMES[0] == "abs_diff"
    names = {"flow": V.FLOW_ERROR_NAMES, "depth": V.DEPTH_ERROR_NAMES}
    p = TR.build_parser()
    n = 0
    for bits in itertools.product((False, True), repeat=4):
        fix = dict(zip(TR.NETS, bits))
        if all(bits):
            continue
        n += 1
        trained = tuple(k for k in TR.NETS if not fix[k])
        which, idx = _reference_choice(fix)
        for with_flow, with_depth in itertools.product((False, True), repeat=2):
            got = TR.decisive_choice(trained, with_flow, with_depth)
            have = with_flow if which == "flow" else with_depth
            assert got == ((which, idx, names[which][idx]) if have else ("unsup", 0, "loss")), (fix, with_flow, with_depth)
            # the same through the flags: the schedule's one phase, and whether the train=False store is needed
            flags = [f for k, f in (("disp", "--fix-dispnet"), ("pose", "--fix-posenet"), ("mask", "--fix-masknet"), ("flow", "--fix-flownet")) if fix[k]]
            a = p.parse_args(["D", "--name", "n"] + flags + (["--with-flow-gt"] if with_flow else []) + (["--with-depth-gt"] if with_depth else []))
            assert TR.schedule(a)[0][1] == trained
            assert TR.needs_unsup_store(a) == ((not with_depth) or not have)
    assert n == 15
    with pytest.raises(ValueError):
        TR.decisive_choice((), True, True)


def test_ledger_capacity_and_step_config():
    for pf, want in ((1, 2), (2, 4), (3, 8), (10, 32), (16, 32), (17, 64)):
        assert TR.ledger_capacity(pf) == want and want >= 2 * pf
    a = TR.build_parser().parse_args(["D", "--name", "n", "-pc", "2", "-m", "0.3", "-s", "0.4", "-pf", "5", "-c", "6", "-wssim", "0.7", "-wrig", "0.8",
                                      "-wbce", "0.9", "--THRESH", "0.2", "-qch", "0.6", "--lambda-oob", "0.1", "--smoothness-type", "edgeaware",
                                      "--spatial-normalize", "--no-non-rigid-mask", "--lr", "0.5", "--momentum", "0.8", "--beta", "0.99",
                                      "--wd", "0.01", "--max-grad-norm", "3"])
    c = TR.step_config(a, 32)
    assert (c.w1, c.w2, c.w3, c.w4, c.w5, c.wssim, c.wrig, c.wbce, c.THRESH, c.qch, c.lambda_oob) == (2, 0.3, 0.4, 5, 6, 0.7, 0.8, 0.9, 0.2, 0.6, 0.1)
    assert (c.smoothness_type, c.spatial_normalize, c.no_non_rigid_mask, c.lr, c.betas, c.weight_decay, c.max_grad_norm, c.ledger) == \
        ("edgeaware", True, True, 0.5, (0.8, 0.99), 0.01, 3.0, 32)


@pytest.mark.slow
def test_one_epoch_end_to_end_emulated(tmp_path):
    import train_cases as C
    from hipemu.emu import emulated_engine
    with emulated_engine():
        C.check_end_to_end("cpu", tmp_path)
