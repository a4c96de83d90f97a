"""``python -m cc_amd.train DATA --name RUN ...``: the reference's ``main()`` and ``train()`` (train.py:141-419, :422-586) on the engine's
parts -- the training set and both validation sets resident in HBM (cc_amd/datasets), the captured step with its ledger
(`CCTrainer`), the store validation passes (cc_amd/validate.py) and the five-file checkpoints (cc_amd/utils.py).  One process, one GPU.

Every option string of train.py:34-135 is accepted with the reference's dest, type, choices and default
(tests/golden/train_args.json, written by tools/make_train_golden.py from the unmodified file).  What differs:

  deviation                                   why
  ------------------------------------------  ---------------------------------------------------------------------------------------
  --posenet / --masknet / --flownet default   the reference's defaults ('PoseNet', 'MaskNet', 'FlowNetS') name no module of `models`
  to PoseNetB6 / MaskNet6 / Back2Future       and fail at train.py:249-255
  --name keeps required=True                  (as the reference; its default 'demo' is never used)
  --robust, --joint-mask-for-depth refused    the reference raises NameError at train.py:431 / :479
  --dataset-format stacked refused            FrameStore reads sequence folders only
  --sequence-length != 5 refused              train.py:463-471 index ref_imgs[1:3], pose[:, 1] and pose[:, 2]
  all four --fix-* refused                    nothing to train; train.py:382-389 leave decisive_error unset
  --flownet FlowNetC6 refused                 the step makes Back2Future's joint call (trainer.cc_forward), not train.py:465-466's two
  frame / --flow-size not a multiple of 64    the six-level networks halve the frame six times
  -f, --log-output, --log-terminal,           accepted, one printed line, no effect: TensorBoard images, the progress bar and flags the
  --alternating, --clamp-masks,               reference itself never reads
  --fix-posemasknet, -e
  -j                                          decode workers of the store builds (there is no DataLoader)
  --resume                                    continues at the checkpoint's epoch and runs up to --epochs in total (the reference
                                              counts from 0 again); the two logs are appended to, not truncated
  no ground truth for the decisive error      the unsupervised total loss of validate_without_gt_from_store decides (the reference
                                              dies with a NameError at :383)
  epoch e draws from seed + e                 `random`, `np.random` and the loader's order: epoch 0 is the reference's, every epoch is a
                                              function of (seed, e) only -- which is what makes --resume exact
  ground-truth passes under                   normalise with mean = std = 0.5 (the resident validation loaders have no local form); the
  --data-normalization local                  training batches and the unsupervised pass follow the flag

Driver-only flags: --phases / --cycles (below), --val-batch-size (8), --flow-size H W (256 832, train.py:163), --store-cache DIR,
--max-grad-norm, --checkpoint-root (checkpoints, train.py:149), --device (cuda; cpu = the x86 emulation build, eager).

Phases (the paper's Algorithm 1): ``--phases "disp+pose:30,flow:30,mask:10" --cycles 3`` trains the named networks for that many
epochs with the others fixed, the list repeated --cycles times; it overrides --fix-* and --epochs.  A network is frozen for good
before a trainer is built, so every phase gets a trainer of its own: at a boundary the checkpoint is on disk, the trainer and its
graph are dropped, `requires_grad` is set for the new set and a fresh `CCTrainer` -- with a FRESH Adam, as a newly started reference
run with other --fix-* flags would have -- is built.  The train transform rotates when 'flow' is trained (train.py:171-185), the
decisive error follows the phase's set, the best error is kept per set, the epoch counter runs on.

Logs: --log-full, one tab-separated row [loss, loss_1, loss_2 or 0, loss_3, loss_4] per step (train.py:574-576), written from the
ledger's drained rows every --print-freq steps; --log-summary, one row [train_loss, decisive_error] per epoch (train.py:415-417);
stdout, one JSON object per epoch.
"""
import argparse
import csv
import gc
import json
import os
import random
import sys
import time

import numpy as np

NETS = ("disp", "pose", "mask", "flow")
FIX_FLAGS = {"disp": "fix_dispnet", "pose": "fix_posenet", "mask": "fix_masknet", "flow": "fix_flownet"}
NO_EFFECT = (("training_output_freq", "-f"), ("log_output", "--log-output"), ("log_terminal", "--log-terminal"),
             ("alternating", "--alternating"), ("clamp_masks", "--clamp-masks"), ("fix_posemasknet", "--fix-posemasknet"),
             ("evaluate", "-e"))
# train.py:382-389: the first network that is trained, in this order, names the error that selects the best checkpoint.  The INDICES
# are the reference's; its comments name the entry before each (flow_errors[-2] is epe_non_rigid_with_gt_mask, [-1] outliers_gt_mask)
DECISIVE = (("pose", "flow", -2), ("disp", "depth", 0), ("flow", "flow", -1), ("mask", "flow", 3))


def build_parser():
    p = argparse.ArgumentParser(prog="python -m cc_amd.train", formatter_class=argparse.ArgumentDefaultsHelpFormatter,
                                description="Competitive Collaboration training on the engine: epochs, validation, checkpoints, phases")
    a = p.add_argument
    a('data', metavar='DIR', help='the prepared training set (sequence folders with train.txt / val.txt)')
    a('--kitti-dir', dest='kitti_dir', type=str, default='kitti/kitti2015', help='KITTI 2015 scene flow tree (flow validation)')
    a('--DEBUG', action='store_true', help='train on the first 32 samples only')
    a('--name', dest='name', type=str, default='demo', required=True, help='run name: checkpoints go to <checkpoint-root>/<name>')
    a('--dataset-format', default='sequential', metavar='STR', help='sequential only')
    a('--sequence-length', type=int, metavar='N', default=5, help='frames per sample (5 only)')
    a('--rotation-mode', type=str, choices=['euler', 'quat'], default='euler', help='accepted; the pose parametrisation is euler')
    a('--padding-mode', type=str, choices=['zeros', 'border'], default='zeros', help='accepted; the warps pad with zeros')
    a('--with-depth-gt', action='store_true', help='validate depth against the .npy ground truth of the validation folders')
    a('--with-flow-gt', action='store_true', help='validate flow against KITTI 2015 (--kitti-dir)')
    a('-j', '--workers', default=4, type=int, metavar='N', help='decode workers of the store builds')
    a('--epochs', default=200, type=int, metavar='N', help='epochs in total')
    a('--epoch-size', default=0, type=int, metavar='N', help='steps per epoch (0: the whole training set)')
    a('-b', '--batch-size', default=4, type=int, metavar='N', help='mini-batch size')
    a('--lr', '--learning-rate', default=2e-4, type=float, metavar='LR', help='learning rate')
    a('--momentum', default=0.9, type=float, metavar='M', help="Adam's beta1")
    a('--beta', default=0.999, type=float, metavar='M', help="Adam's beta2")
    a('--weight-decay', '--wd', default=0, type=float, metavar='W', help='weight decay')
    a('--print-freq', default=10, type=int, metavar='N', help='steps between two reads of the step ledger')
    a('-e', '--evaluate', dest='evaluate', action='store_true', help='no effect')
    a('--smoothness-type', dest='smoothness_type', type=str, default='regular', choices=['edgeaware', 'regular'], help='smoothness term')
    a('--data-normalization', dest='data_normalization', type=str, default='global', choices=['local', 'global'],
      help='mean = std = 0.5, or per-sample statistics')
    a('--nlevels', dest='nlevels', type=int, default=6, help='levels of the flow network')
    a('--dispnet', dest='dispnet', type=str, default='DispNetS', choices=['DispNetS', 'DispNetS6', 'DispResNetS6', 'DispResNet6'],
      help='depth network')
    a('--posenet', dest='posenet', type=str, default='PoseNetB6', choices=['PoseNet6', 'PoseNetB6', 'PoseExpNet'], help='pose network')
    a('--masknet', dest='masknet', type=str, default='MaskNet6', choices=['MaskResNet6', 'MaskNet6'], help='mask network')
    a('--flownet', dest='flownet', type=str, default='Back2Future', choices=['Back2Future', 'FlowNetC6'], help='flow network')
    a('--pretrained-disp', dest='pretrained_disp', default=None, metavar='PATH', help='depth network checkpoint')
    a('--pretrained-mask', dest='pretrained_mask', default=None, metavar='PATH', help='mask network checkpoint')
    a('--pretrained-pose', dest='pretrained_pose', default=None, metavar='PATH', help='pose network checkpoint')
    a('--pretrained-flow', dest='pretrained_flow', default=None, metavar='PATH', help='flow network checkpoint')
    a('--spatial-normalize', dest='spatial_normalize', action='store_true', help='divide every disparity level by its mean')
    a('--robust', dest='robust', action='store_true', help='refused')
    a('--no-non-rigid-mask', dest='no_non_rigid_mask', action='store_true', help='flow photometric loss without the mask')
    a('--joint-mask-for-depth', dest='joint_mask_for_depth', action='store_true', help='refused')
    a('--fix-masknet', dest='fix_masknet', action='store_true', help='do not train the mask network')
    a('--fix-posenet', dest='fix_posenet', action='store_true', help='do not train the pose network')
    a('--fix-flownet', dest='fix_flownet', action='store_true', help='do not train the flow network')
    a('--fix-dispnet', dest='fix_dispnet', action='store_true', help='do not train the depth network')
    a('--alternating', dest='alternating', action='store_true', help='no effect')
    a('--clamp-masks', dest='clamp_masks', action='store_true', help='no effect')
    a('--fix-posemasknet', dest='fix_posemasknet', action='store_true', help='no effect')
    a('--seed', default=0, type=int, help='seed of the initialisation, the order and the augmentation')
    a('--log-summary', default='progress_log_summary.csv', metavar='PATH', help='per-epoch log, under the checkpoint directory')
    a('--log-full', default='progress_log_full.csv', metavar='PATH', help='per-step log, under the checkpoint directory')
    a('-qch', '--qch', type=float, metavar='W', default=0.5, help='Charbonnier exponent')
    a('-wrig', '--wrig', type=float, metavar='W', default=1.0, help='consensus imbalance weight')
    a('-wbce', '--wbce', type=float, metavar='W', default=0.5, help='weight of the cross entropy')
    a('-wssim', '--wssim', type=float, metavar='W', default=0.0, help='weight of SSIM in the photometric terms')
    a('-pc', '--cam-photo-loss-weight', type=float, metavar='W', default=1, help='w1: rigid photometric loss')
    a('-pf', '--flow-photo-loss-weight', type=float, metavar='W', default=1, help='w4: flow photometric loss')
    a('-m', '--mask-loss-weight', type=float, metavar='W', default=0, help='w2: mask regulariser')
    a('-s', '--smooth-loss-weight', type=float, metavar='W', default=0.1, help='w3: smoothness')
    a('-c', '--consensus-loss-weight', type=float, metavar='W', default=0.1, help='w5: consensus')
    a('--THRESH', '--THRESH', type=float, metavar='W', default=0.01, help='mask threshold')
    a('--lambda-oob', type=float, default=0, help='weight of the out-of-bound pixels')
    a('--log-output', action='store_true', help='no effect')
    a('--log-terminal', action='store_true', help='no effect')
    a('--resume', action='store_true', help="continue from the run's checkpoint")
    a('-f', '--training-output-freq', type=int, metavar='N', default=0, help='no effect')
    g = p.add_argument_group("driver")
    g.add_argument('--phases', default=None, metavar='SPEC', help='e.g. "disp+pose:30,flow:30,mask:10": trained networks and epochs per phase')
    g.add_argument('--cycles', default=1, type=int, metavar='N', help='repetitions of the --phases list')
    g.add_argument('--val-batch-size', default=8, type=int, metavar='N', help='batch size of the validation passes')
    g.add_argument('--flow-size', default=[256, 832], type=int, nargs=2, metavar=('H', 'W'), help='frame size of the flow validation')
    g.add_argument('--store-cache', default=None, metavar='DIR', help='save / load the decoded stores here')
    g.add_argument('--max-grad-norm', default=None, type=float, metavar='G', help='gradient guard of the step (clip per network)')
    g.add_argument('--checkpoint-root', default='checkpoints', metavar='DIR', help='parent of the run directory')
    g.add_argument('--device', default='cuda', help='cuda, or cpu (the x86 emulation build)')
    return p


# ----------------------------------------------------------------------------------------------------------------- phases
def parse_phases(spec):
    """"disp+pose:30,flow:30" -> [(("disp", "pose"), 30), (("flow",), 30)]: names in chain order; ValueError says what is wrong"""
    out = []
    for part in str(spec).split(","):
        names, sep, n = part.strip().partition(":")
        if not sep or not names.strip() or not n.strip():
            raise ValueError("--phases: %r is not NETS:EPOCHS (e.g. disp+pose:30)" % part.strip())
        got = [s.strip() for s in names.split("+")]
        bad = [s for s in got if s not in NETS]
        if bad:
            raise ValueError("--phases: unknown network %r in %r (known: %s)" % (bad[0], part.strip(), ", ".join(NETS)))
        if len(set(got)) != len(got):
            raise ValueError("--phases: a network is named twice in %r" % part.strip())
        try:
            epochs = int(n)
        except ValueError:
            raise ValueError("--phases: %r epochs in %r" % (n.strip(), part.strip()))
        if epochs < 1:
            raise ValueError("--phases: %d epochs in %r" % (epochs, part.strip()))
        out.append((tuple(k for k in NETS if k in got), epochs))
    return out


def schedule(args):
    """-> [(cycle, trained names, first epoch, end epoch)]: the --phases list --cycles times, or the one phase of --fix-* / --epochs"""
    if args.phases is None:
        return [(0, tuple(k for k in NETS if not getattr(args, FIX_FLAGS[k])), 0, args.epochs)]
    out, e = [], 0
    for c in range(args.cycles):
        for names, n in parse_phases(args.phases):
            out.append((c, names, e, e + n))
            e += n
    return out


def decisive_choice(trained, with_flow_gt, with_depth_gt):
    """train.py:382-389 -> (pass, index, name): pass 'flow' / 'depth' / 'unsup' and the index into that pass's errors.  Where the
    ground-truth pass of the reference's choice did not run, the unsupervised total loss decides."""
    from .validate import DEPTH_ERROR_NAMES, FLOW_ERROR_NAMES
    for net, which, idx in DECISIVE:
        if net in trained:
            if which == "flow" and with_flow_gt:
                return "flow", idx, FLOW_ERROR_NAMES[idx]
            if which == "depth" and with_depth_gt:
                return "depth", idx, DEPTH_ERROR_NAMES[idx]
            return "unsup", 0, "loss"
    raise ValueError("no network is trained")


def needs_unsup_store(args):
    """train.py:208-215 builds the train=False sequence set when there is no depth ground truth; a phase whose decisive error has
    no ground-truth pass needs it too"""
    return (not args.with_depth_gt) or any(decisive_choice(names, args.with_flow_gt, args.with_depth_gt)[0] == "unsup"
                                           for _, names, _, _ in schedule(args))


def launched_world_size(world_size=None):
    """How many processes this run is part of.  The package reads nothing from the process environment (tests/test_abi.py), so a
    launcher's WORLD_SIZE reaches the driver the way every other setting does -- as an argument (`main(argv, world_size=)`, from
    the script that starts it) -- or through torch.distributed: an initialised process group says its size, and a process started
    by torchrun (torch.distributed.is_torchelastic_launched) counts as one of several whatever --nproc-per-node was: a single
    process needs no launcher."""
    import torch.distributed as dist
    if world_size is not None:
        return int(world_size), "world_size = %d" % int(world_size)
    if dist.is_available() and dist.is_initialized():
        return dist.get_world_size(), "a process group of %d ranks is initialised" % dist.get_world_size()
    if dist.is_available() and dist.is_torchelastic_launched():
        return 2, "started by torchrun"
    return 1, ""


def check_args(p, args, world_size=None):
    """the refusals that need the command line only (SystemExit through parser.error)"""
    world, how = launched_world_size(world_size)
    if world > 1:
        p.error("%s: this driver is one process on one GPU (WORLD_SIZE 1); the data-parallel launcher is not part of it" % how)
    if args.robust:
        p.error("--robust: the reference names photometric_reconstruction_loss_robust, which does not exist (train.py:431)")
    if args.joint_mask_for_depth:
        p.error("--joint-mask-for-depth: the reference calls compute_joint_mask_for_depth without its THRESH argument (train.py:479)")
    if args.dataset_format != "sequential":
        p.error("--dataset-format %s: the resident FrameStore reads sequence folders only" % args.dataset_format)
    if args.sequence_length != 5:
        p.error("--sequence-length %d: the step indexes ref_imgs[1:3], pose[:, 1] and pose[:, 2] (train.py:463-471), which is "
                "a sequence of 5" % args.sequence_length)
    if args.flownet != "Back2Future":
        p.error("--flownet %s: the step makes Back2Future's joint forward / backward call" % args.flownet)
    if any(v % 64 or v <= 0 for v in args.flow_size):
        p.error("--flow-size %d %d: height and width must be multiples of 64" % tuple(args.flow_size))
    if args.batch_size < 1 or args.val_batch_size < 1 or args.print_freq < 1 or args.cycles < 1:
        p.error("--batch-size, --val-batch-size, --print-freq and --cycles must be at least 1")
    if args.phases is None:
        if args.cycles != 1:
            p.error("--cycles needs --phases")
        if all(getattr(args, f) for f in FIX_FLAGS.values()):
            p.error("all four --fix-* flags: nothing to train (and train.py:382-389 would leave decisive_error unset)")
    else:
        try:
            parse_phases(args.phases)
        except ValueError as e:
            p.error(str(e))


def check_frame_size(p, args):
    """a frame height or width that is not a multiple of 64 is refused before anything is decoded (the first frame's header)"""
    from PIL import Image
    from .datasets import crawl
    _, _, found = crawl(args.data, True, args.sequence_length)
    if not found:
        p.error("%s: no scene with %d or more frames" % (args.data, args.sequence_length))
    with Image.open(found[0][1][0]) as im:
        W, H = im.size
    if H % 64 or W % 64:
        p.error("%s: frames of %d x %d; height and width must be multiples of 64 (the six-level networks halve them six times)"
                % (args.data, H, W))


# ----------------------------------------------------------------------------------------------------------------- set-up
def step_config(args, capacity=None):
    from .trainer import StepConfig
    return StepConfig(w1=args.cam_photo_loss_weight, w2=args.mask_loss_weight, w3=args.smooth_loss_weight, w4=args.flow_photo_loss_weight,
                      w5=args.consensus_loss_weight, wssim=args.wssim, wrig=args.wrig, wbce=args.wbce, THRESH=args.THRESH, qch=args.qch,
                      lambda_oob=args.lambda_oob, smoothness_type=args.smoothness_type, spatial_normalize=args.spatial_normalize,
                      no_non_rigid_mask=args.no_non_rigid_mask, lr=args.lr, betas=(args.momentum, args.beta),
                      weight_decay=args.weight_decay, max_grad_norm=args.max_grad_norm, ledger=capacity)


def ledger_capacity(print_freq):
    """a power of two that is at least 2 * print_freq: a drain every print_freq steps never meets an overwritten row"""
    return 1 << max(1, (2 * int(print_freq) - 1).bit_length())


def _cached(cls, directory, build):
    """--store-cache: load the store from `directory` when it is there, else build it and save it there"""
    if directory is None:
        return build()
    if os.path.isfile(os.path.join(directory, "store.json")):
        return cls.load(directory)
    store = build()
    store.save(directory)
    return store


def build_stores(args, dev):
    """train.py:192-224 -> (train, depth_val or None, flow_val or None, unsup_val or None), all resident on `dev`"""
    from . import datasets as DS
    from .kitti_eval import Kitti2015Flow
    sub = (lambda name: os.path.join(args.store_cache, name)) if args.store_cache else (lambda name: None)
    L, w = args.sequence_length, args.workers

    class _On(object):          # (the stores' load() takes the device as a keyword too)
        def __init__(self, cls):
            self.cls = cls

        def load(self, d):
            return self.cls.load(d, device=dev)

    print("=> fetching scenes in '{}'".format(args.data), file=sys.stderr)
    train = _cached(_On(DS.FrameStore), sub("train"), lambda: DS.FrameStore.build(args.data, train=True, sequence_length=L, device=dev, workers=w))
    if args.DEBUG and len(train) > 32:                                       # :222-224
        train = DS.FrameStore(train.frames, train.minmax, train.intrinsics, train.samples[:32], train.sample_scene[:32], train.scenes)
    depth = flow = unsup = None
    if args.with_depth_gt:
        root = args.data.replace('cityscapes', 'kitti')                      # :205
        depth = _cached(_On(DS.DepthValStore), sub("val_depth"), lambda: DS.DepthValStore.build(root, device=dev, workers=w))
    if args.with_flow_gt:
        def build_flow():
            # (the reference reads samples 000000 .. 000199; here: as many as the tree holds ground truth for, in that numbering)
            fw = Kitti2015Flow(args.kitti_dir, sequence_length=L)
            n = 0
            while n < fw.N and fw.paths(n)['flow'].is_file():
                n += 1
            if n == 0:
                raise ValueError("%s: no KITTI 2015 flow ground truth (%s)" % (args.kitti_dir, fw.paths(0)['flow']))
            fw.N = n
            return DS.FlowValStore.build(fw, tuple(args.flow_size), device=dev)
        flow = _cached(_On(DS.FlowValStore), sub("val_flow"), build_flow)
    if needs_unsup_store(args):
        unsup = _cached(_On(DS.FrameStore), sub("val_unsup"),
                        lambda: DS.FrameStore.build(args.data, train=False, sequence_length=L, device=dev, workers=w))
    print('{} samples found in {} train scenes'.format(len(train), len(train.scenes)), file=sys.stderr)
    return train, depth, flow, unsup


def build_networks(args, dev):
    """train.py:245-284: constructor arguments, pretrained weights or init_weights(), in the reference's order"""
    import torch
    from . import models, utils
    L = args.sequence_length
    disp_net = getattr(models, args.dispnet)().to(dev)
    pose_net = getattr(models, args.posenet)(nb_ref_imgs=L - 1).to(dev)
    mask_net = getattr(models, args.masknet)(nb_ref_imgs=L - 1, output_exp=True).to(dev)
    flow_net = getattr(models, args.flownet)(nlevels=args.nlevels).to(dev)
    for net, path in ((pose_net, args.pretrained_pose), (mask_net, args.pretrained_mask), (disp_net, args.pretrained_disp),
                      (flow_net, args.pretrained_flow)):
        if path:
            utils.load_pretrained(net, path, map_location=dev)
        else:
            net.init_weights()
    return [disp_net, pose_net, mask_net, flow_net]


def make_trainer(args, nets, trained, dev):
    """requires_grad for the phase's set BEFORE the trainer exists (a network is frozen for good by it), then the trainer in its
    default form: captured on a HIP device, eager on the emulation"""
    from .trainer import CCTrainer
    for name, n in zip(NETS, nets):
        for q in n.parameters():
            q.requires_grad = name in trained
    return CCTrainer(nets, step_config(args, ledger_capacity(args.print_freq)), use_graph=dev.type == "cuda")


# ----------------------------------------------------------------------------------------------------------------- one epoch
def train_epoch(tr, loader, n_steps, print_freq, log_full=None, epoch=0):
    """train.py:445-586 for one epoch: n_steps steps of tr.step(batch) without a host read per step; the ledger is drained every
    print_freq steps and at the end, its rows appended to `log_full`.  -> (steps, train_loss).  A drained row with the NaN flag set
    stops the run and names the step; rows lost to the ring (`dropped`) are an error."""
    for n in tr.nets:
        n.train()                                                            # :438-441
    led = tr.ledger

    def drain():
        d = led.drain()
        if d.dropped:
            raise RuntimeError("step ledger: %d rows were overwritten before they were read (capacity %d, print_freq %d)"
                               % (d.dropped, led.capacity, print_freq))
        bad = (d.rows[:, 7] != 0).nonzero()
        if bad.numel():
            k = int(bad[0])
            raise FloatingPointError("NaN in a photometric loss term at step %d (epoch %d, iteration %d of this trainer)"
                                     % (int(d.rows[k, 0]), epoch, d.first_iter + k))
        if log_full is not None and d.rows.shape[0]:
            led.write_log_full(log_full, d.rows)

    done = 0
    for batch in loader:
        tr.step(batch)
        done += 1
        if done % print_freq == 0:
            drain()
        if done >= n_steps:                                                  # :581
            break
    drain()
    train_loss = led.average()['loss']['avg']                                # :586 losses.avg[0]
    led.reset_average()
    return done, train_loss


def validate_epoch(args, nets, stores, cfg):
    """-> {'flow': (errors, names), 'depth': .., 'unsup': ..} for the passes whose store exists (train.py:360-364)"""
    from . import validate as V
    _, depth, flow, unsup = stores
    out = {}
    if flow is not None:
        out["flow"] = V.validate_flow_from_store(flow, *nets, batch_size=args.val_batch_size, args=args)
    if depth is not None:
        out["depth"] = V.validate_depth_from_store(depth, nets[0], args.val_batch_size, args=args)
    if unsup is not None:
        out["unsup"] = V.validate_without_gt_from_store(unsup, *nets, args.val_batch_size, cfg, normalize=args.data_normalization)
    return out


def main(argv=None, world_size=None):
    """world_size: the launcher's WORLD_SIZE, where the caller knows one (launched_world_size); more than one process is refused"""
    p = build_parser()
    args = p.parse_args(argv)
    check_args(p, args, world_size)
    check_frame_size(p, args)
    import torch
    from . import utils
    from .custom_transforms import DeviceTrainTransform
    from .datasets import DeviceSequenceLoader
    for dest, flag in NO_EFFECT:
        if getattr(args, dest):
            print("=> %s is accepted and has no effect" % flag, file=sys.stderr)
    dev = torch.device(args.device)
    args.save_path = os.path.join(args.checkpoint_root, args.name)           # :148-151
    print('=> will save everything to {}'.format(args.save_path), file=sys.stderr)
    os.makedirs(args.save_path, exist_ok=True)
    torch.manual_seed(args.seed)                                             # :152

    stores = build_stores(args, dev)
    nets = build_networks(args, dev)
    start = 0
    if args.resume:                                                          # :286-295
        start = int(utils.resume(args.save_path, *nets, map_location=dev) or 0)
        print("=> resuming from checkpoint at epoch %d" % start, file=sys.stderr)
    plan = schedule(args)
    total = plan[-1][3]

    log_summary, log_full = os.path.join(args.save_path, args.log_summary), os.path.join(args.save_path, args.log_full)
    for path, header in ((log_summary, ['train_loss', 'validation_loss']),
                         (log_full, ['train_loss', 'photo_cam_loss', 'photo_flow_loss', 'explainability_loss', 'smooth_loss'])):
        if not (args.resume and os.path.isfile(path)):                       # :317-323
            with open(path, 'w') as f:
                csv.writer(f, delimiter='\t').writerow(header)

    best = {}                                   # trained set -> best decisive error so far (-1: none yet, train.py:137)
    tr = None
    for cycle, trained, first, end in plan:
        if end <= start:
            continue
        # ---- a phase: its own trainer, loader and decisive error
        if tr is not None:                      # a phase boundary: the trainer with its graph goes, nothing of it stays on the device
            tr.close()
            tr = None
            gc.collect()
            if dev.type == "cuda":
                torch.cuda.empty_cache()
        tr = make_trainer(args, nets, trained, dev)
        if args.resume and start > first:                                    # :312-315 -- inside a phase only: a new phase starts with a fresh Adam
            utils.resume_optimizer(args.save_path, tr, map_location=dev)
        transform = DeviceTrainTransform(device=dev, rotate="flow" in trained, normalize=args.data_normalization)   # :171-185
        loader = DeviceSequenceLoader(stores[0], args.batch_size, transform, seed=args.seed)
        n_steps = min(len(loader), args.epoch_size) if args.epoch_size else len(loader)     # :239-240, :581
        if n_steps < 1:
            raise ValueError("%d training samples give no batch of %d" % (len(stores[0]), args.batch_size))
        which, idx, dname = decisive_choice(trained, args.with_flow_gt, args.with_depth_gt)
        for epoch in range(max(first, start), end):
            t0 = time.time()
            random.seed(args.seed + epoch)
            np.random.seed(args.seed + epoch)
            loader.set_epoch(epoch)
            steps, train_loss = train_epoch(tr, loader, n_steps, args.print_freq, log_full, epoch)
            val = validate_epoch(args, nets, stores, tr.cfg)
            decisive_error = val[which][0][idx]
            key = frozenset(trained)
            best_error = best.get(key, -1)
            if best_error < 0:                                               # :390-395
                best_error = decisive_error
            is_best = bool(decisive_error <= best_error)
            best[key] = min(best_error, decisive_error)
            tr.save_checkpoint(args.save_path, epoch, is_best)               # :396-413 ('epoch': epoch + 1)
            with open(log_summary, 'a') as f:
                csv.writer(f, delimiter='\t').writerow([train_loss, decisive_error])
            line = {"epoch": epoch, "epochs": total, "cycle": cycle, "phase": "+".join(trained), "steps": steps, "train_loss": train_loss}
            for kind in ("flow", "depth", "unsup"):
                if kind in val:
                    errors, names = val[kind]
                    line.update({("val_" + n if kind == "unsup" else n): v for n, v in zip(names, errors)})
            line.update(decisive=("val_" + dname if which == "unsup" else dname), decisive_error=decisive_error, is_best=is_best,
                        seconds=round(time.time() - t0, 3))
            print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
