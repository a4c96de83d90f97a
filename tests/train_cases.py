"""Shared cases of the training driver (cc_amd/train.py): the 64 x 128 trees (built with the helpers of tests/frame_store_cases.py and
tests/validation_store_cases.py), seeded start weights as --pretrained-* files, a runner that collects the driver's JSON lines, and
the checks that run on the x86 emulation build (dev = "cpu") and on the GPU (dev = "cuda") alike.  64 x 128 at B = 2 is the smallest
size the six-level step runs at in this suite (tests/loss_calls.py: LB, LH, LW)."""
import contextlib
import csv
import io
import json
import os

import torch

import frame_store_cases as FC
from cc_amd import synthetic as syn, train as TR, trainer as T, utils
from loss_calls import LB, LH, LW

CKPT_FILES = ["%s_checkpoint.pth.tar" % p for p in utils.FILE_PREFIXES]
FULL_HEADER = ['train_loss', 'photo_cam_loss', 'photo_flow_loss', 'explainability_loss', 'smooth_loss']
SUMMARY_HEADER = ['train_loss', 'validation_loss']


def data_tree(tmp, name="data"):
    """5 training samples (two steps of B = 2 per epoch) and 2 validation samples (scene_b) of five 64 x 128 frames"""
    return FC.build_tree(os.path.join(str(tmp), name), LH, LW)


def seeded_nets(dev):
    nets = T.build_nets(dev, init=False)
    for n in nets:
        n.load_state_dict(syn.seeded_state_dict(n, 0))
    return nets


def seeded_files(tmp):
    """the seeded start weights in the checkpoint wire format -> the --pretrained-* arguments"""
    d = os.path.join(str(tmp), "pretrained")
    os.makedirs(d, exist_ok=True)
    out = []
    for name, n in zip(("disp", "pose", "mask", "flow"), T.build_nets("cpu", init=False)):
        path = os.path.join(d, name + ".pth.tar")
        if not os.path.isfile(path):
            torch.save({"epoch": 0, "state_dict": syn.seeded_state_dict(n, 0)}, path)
        out += ["--pretrained-" + name, path]
    return out


def argv(tmp, root, name, dev, *extra):
    """(edge-aware smoothness: the reference's 'regular' term takes second differences, which are empty -- a NaN mean, in the
    reference too -- at the 2 x 4 and 1 x 2 levels of a 64 x 128 frame)"""
    return [root, "--name", name, "--checkpoint-root", os.path.join(str(tmp), "ck"), "--dispnet", "DispResNet6", "-b", str(LB),
            "-j", "2", "--device", dev, "--smoothness-type", "edgeaware"] + seeded_files(tmp) + list(extra)


def run(args):
    """main(args) -> the JSON lines it printed"""
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        assert TR.main(args) == 0
    return [json.loads(line) for line in buf.getvalue().splitlines() if line.startswith("{")]


def save_path(tmp, name):
    return os.path.join(str(tmp), "ck", name)


def read_tsv(path):
    with open(path) as f:
        return list(csv.reader(f, delimiter='\t'))


def load_checkpoints(path, kind="checkpoint"):
    return [torch.load(os.path.join(path, "%s_%s.pth.tar" % (p, kind)), map_location="cpu") for p in utils.FILE_PREFIXES]


def tensors_of(obj, prefix=""):
    """every tensor of a nested checkpoint, by path"""
    if torch.is_tensor(obj):
        yield prefix, obj
    elif isinstance(obj, dict):
        for k in obj:
            yield from tensors_of(obj[k], "%s/%s" % (prefix, k))
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            yield from tensors_of(v, "%s/%d" % (prefix, i))


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float32:
        return torch.equal(a.view(torch.int32), b.view(torch.int32))
    return torch.equal(a, b)


def check_end_to_end(dev, tmp):
    """one epoch of one step plus the unsupervised pass: the five checkpoint files (loadable into fresh networks), both TSVs with
    their header rows, one JSON line"""
    root = data_tree(tmp)
    lines = run(argv(tmp, root, "e2e", dev, "--epochs", "1", "--epoch-size", "1"))
    sp = save_path(tmp, "e2e")
    assert sorted(f for f in os.listdir(sp) if f.endswith("_checkpoint.pth.tar")) == sorted(CKPT_FILES)
    cks = load_checkpoints(sp)
    assert all(c["epoch"] == 1 for c in cks)
    nets = T.build_nets("cpu", init=False)
    start = seeded_nets("cpu")
    for n, s, c in zip(nets, start, cks[:4]):
        n.load_state_dict(c["state_dict"])
        assert any(not torch.equal(a, b) for a, b in zip(n.parameters(), s.parameters()))       # the step trained it
    assert set(cks[4]["state_dict"]) == {"state", "param_groups"} and len(cks[4]["state_dict"]["state"]) == sum(len(list(n.parameters())) for n in nets)
    full, summary = read_tsv(os.path.join(sp, "progress_log_full.csv")), read_tsv(os.path.join(sp, "progress_log_summary.csv"))
    assert full[0] == FULL_HEADER and len(full) == 2 and len(full[1]) == 5 and full[1][2] == "0"            # -m 0: loss_2 is the integer 0
    assert summary[0] == SUMMARY_HEADER and len(summary) == 2
    assert len(lines) == 1
    ln = lines[0]
    assert (ln["epoch"], ln["steps"], ln["phase"], ln["decisive"], ln["is_best"]) == (0, 1, "disp+pose+mask+flow", "val_loss", True)
    assert float(summary[1][0]) == ln["train_loss"] == float(full[1][0]), (summary[1], ln, full[1])        # one step: its loss is the mean
    assert float(summary[1][1]) == ln["decisive_error"] == ln["val_loss"], (summary[1], ln)
    assert all(0 < abs(ln["val_" + k]) < 1e3 for k in ("loss", "loss_1", "loss_3", "loss_4", "loss_5"))
    assert os.path.isfile(os.path.join(sp, "dispnet_model_best.pth.tar"))
    return ln
