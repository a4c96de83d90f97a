"""The conv-family engine calls (convolutions, activation backward / bias sums, batch norm, x2 up-sampling, the 9x9 cost volume)
of three workloads, all at batch 2, logged with tests/loss_calls.py's ArgLog:
  tape   : forward + backward of the four hot networks as tests/test_nets_emu.py::_run drives them (the tape of cc_amd/tape.py);
  step   : one eager CCTrainer.step at 2 x 64 x 128 (the weight-gradient queue, the parked reductions, park_bias, the list call);
  layers : forward + backward of the alternative architectures (tests/test_alt_nets.py) and the config-1 step of
           tests/test_configs_engine.py with the optimizer's gradient sinks and the weight-gradient queue switched on -- the
           per-layer path of cc_amd/ops.py.
tests/golden/conv_calls.json.gz (4603 calls, 380 KB of JSON, one call per line: kept compressed) pins the three sequences
(tests/test_conv_calls.py); it was recorded on the commit BEFORE the launchers of cc_amd/ops.py existed.  `python tests/conv_calls.py` (x86 emulation build) rewrites it, `--bits FILE` also saves
every tensor the workloads produce (outputs, gradients, losses) for a torch.equal comparison between two trees."""
import ctypes
import gzip
import json
import os

import torch

from cc_amd import loss_functions as LF, models, ops, synthetic as syn, trainer as T
from cc_amd._lib import engine
from cc_amd.step_scope import StepScope
from loss_calls import ArgLog
from oracle.make_golden import ALT_NETS, AB, AH, AW, SB, SH, SW, alt_net_args

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_calls.json.gz")
FAMILIES = ("cc_conv2d_", "cc_act_bwd_", "cc_bias_grad_", "cc_wgrad_reduce_table", "cc_repack_table", "cc_bn_", "cc_upsample2x_",
            "cc_corr9x9_")
MEMBERS = {"x", "w", "bias", "res", "y", "prepacked", "gy", "gx", "mul", "add", "geff", "gbias", "a", "gw"}
# the four hot networks: (class, constructor arguments, call form, H, W) -- tests/test_nets_emu.py CASES and sizes
TAPE_NETS = {"disp": (models.DispResNet6, (), "t", 64, 96), "pose": (models.PoseNetB6, (4,), "tr", 64, 96),
             "mask": (models.MaskNet6, (4,), "tr", 64, 128), "flow": (models.Back2Future, (6,), "t2", 64, 128)}


class ConvLog(ArgLog):
    """ArgLog of the conv families.  A HOST address array of a group call (first argument G) is logged as one "p" / 0 per member,
    the descriptors of cc_conv2d_wgrad_list as rows with their addresses replaced the same way; out-parameters and the parked
    tables (host addresses) are "p".  While it is active cc_conv2d_wgrad_ws_bytes is asked on every call, as the tools /
    emulation builds do (the product library memoises it per geometry: the log would depend on what ran before)."""

    def __enter__(self):
        super().__enter__()
        self.was_tools = getattr(self.e, "_is_tools", None)
        self.e._is_tools = True
        return self

    def __exit__(self, *a):
        self.e._is_tools = self.was_tools
        return super().__exit__(*a)

    def keeps(self, name):
        return name.startswith(FAMILIES)

    def arg(self, name, a, v, ty, an):
        names = self.e.sigs[name][2]
        if names[0] == "G" and an in MEMBERS and isinstance(v, int) and v != 0:
            return [("p" if p else 0) for p in (ctypes.c_long * a[0]).from_address(v)]
        if name == "cc_conv2d_wgrad_list" and an == "desc_host":
            tab = (ctypes.c_long * (32 * a[0])).from_address(v)
            return [[("p" if tab[32 * j + k] else 0) if 1 <= k <= 13 else int(tab[32 * j + k]) for k in range(32)] for j in range(a[0])]
        if ty is ctypes.c_void_p:
            return 0 if (v is None or (isinstance(v, int) and v == 0)) else "p"
        return v


def group_spelling(calls):
    """The normalisation of the `layers` trace: a single-problem call (cc_conv2d_fwd, cc_conv2d_dgrad, their *_ws_bytes) is
    written as its group spelling with G = 1 and one-element member lists.  In every group call a member list without an address
    is 0 like the null array, and the batch stride of an absent operand (res, mul) is 0."""
    sigs = engine().sigs
    out = []
    for name, r in calls:
        r = list(r)
        if name in ("cc_conv2d_fwd_ws_bytes", "cc_conv2d_dgrad_ws_bytes"):
            name, r = name.replace("_ws_bytes", "_group_ws_bytes"), [1] + r
        elif name == "cc_conv2d_fwd":           # x, w, bias, res, y, ws, prepacked, ...
            name, r = "cc_conv2d_fwd_group", [1] + [[v] for v in r[:5]] + [r[5], [r[6]]] + r[7:]
        elif name == "cc_conv2d_dgrad":         # gy, w, bias, gx, ws, prepacked, B .. gx_bs, w_k_stride ...
            name, r = "cc_conv2d_dgrad_group", [1] + [[v] for v in r[:4]] + [0, r[4], [r[5]]] + r[6:19] + [0] + r[19:]
        if name in ("cc_conv2d_fwd_group", "cc_conv2d_dgrad_group"):
            names = [n for n in sigs[name][2] if n != "stream"]
            d = {n: (0 if isinstance(v, list) and not any(v) else v) for n, v in zip(names, r)}
            for op in ("res", "mul"):
                if op in d and d[op] == 0:
                    d[op + "_bs"] = 0
            r = [d[n] for n in names]
        out.append([name, r])
    return out


def _flat(o):
    if torch.is_tensor(o):
        return [o]
    return [t for x in o if x is not None for t in _flat(x)]


def _net_pass(net, args, wrt, seed=3):
    """forward (training mode) + backward under seeded output gradients -> [outputs, parameter gradients, gradients of wrt]"""
    outs = _flat(net(*args))
    gen = torch.Generator().manual_seed(seed)
    go = [torch.randn(o.shape, generator=gen).to(o.device) for o in outs]
    sum((o * g).sum() for o, g in zip(outs, go)).backward()
    grads = [p.grad if p.grad is not None else torch.zeros(()) for p in net.parameters()] + [t.grad for t in wrt]
    return [t.detach().clone() for t in outs + grads]


def trace_tape(dev, name):
    """-> (tensors, calls) of one of the four hot networks: training pass, then the eval / no_grad pass (no tape)"""
    cls, cargs, form, H, W = TAPE_NETS[name]
    tgt, refs, K, Kinv = syn.sample(2, H, W, seed=1)
    net = cls(*cargs)
    net.load_state_dict(syn.seeded_state_dict(net, 0))
    net.to(dev)
    t, refs = tgt.clone().to(dev).requires_grad_(name == "disp"), [r.to(dev) for r in refs]
    args = {"t": (t,), "tr": (t, refs), "t2": (t, refs[1:3])}[form]
    ops.packs.reset()
    with ConvLog() as log:
        tensors = _net_pass(net, args, [t] if name == "disp" else [])
        net.eval()
        with torch.no_grad():
            tensors += [o.clone() for o in _flat(net(*args))]
    return tensors, log.calls


def trace_step(dev="cpu"):
    """-> (tensors, calls) of one eager CCTrainer.step at 2 x 64 x 128 (tests/test_step_emu.py::test_full_cc_step_matches_oracle)"""
    batch = syn.sample(2, 64, 128, seed=1)
    batch = (batch[0].to(dev), [r.to(dev) for r in batch[1]], batch[2].to(dev), batch[3].to(dev))
    nets = T.build_nets(dev, init=False)
    for n in nets:
        n.load_state_dict(syn.seeded_state_dict(n, 0))
    tr = T.CCTrainer(nets, T.StepConfig(), use_graph=False)
    with ConvLog() as log:
        losses = tr.step(batch)
    tensors = [losses[k].detach().clone() for k in sorted(losses)] + [tr.opt.flat_g.clone(), tr.opt.flat_p.clone()]
    ops.packs.reset()
    return tensors, log.calls


def trace_alt(dev, name, kw):
    """-> (tensors, calls) of one alternative architecture at its fixture size (tests/test_alt_nets.py: per-layer autograd)"""
    tgt, refs, K, Kinv = syn.sample(AB, AH, AW, seed=1)
    net = getattr(models, name)(**kw)
    net.load_state_dict(syn.seeded_state_dict(net, 0))
    net.to(dev).train()
    ops.packs.reset()
    with ConvLog() as log:
        tensors = _net_pass(net, alt_net_args(name, tgt.to(dev), [r.to(dev) for r in refs]), [])
    return tensors, log.calls


def trace_config1(dev):
    """-> (tensors, calls) of the config-1 step of tests/test_configs_engine.py (DispNetS + PoseExpNet, one scale, photometric +
    smoothness loss) with the parameters in a FlatAdam bucket: the kernels accumulate into its gradient sinks, the weight
    gradients go through the queue, the second stages are parked -- as inside a trainer step, on the per-layer path."""
    tgt, refs, K, Kinv = syn.sample(SB, SH, SW, seed=1)
    dn, pn = models.DispNetS(), models.PoseExpNet(nb_ref_imgs=4, output_exp=False)
    for n in (dn, pn):
        n.load_state_dict(syn.seeded_state_dict(n, 0))
        n.to(dev).train()
    opt = T.FlatAdam([dn, pn], T.StepConfig())
    opt.zero_grad()
    tgt, refs, K, Kinv = tgt.to(dev), [r.to(dev) for r in refs], K.to(dev), Kinv.to(dev)
    try:
        with StepScope(sinks=opt.sinks) as scope, ConvLog() as log:
            disp = dn(tgt)
            exp, pose = pn(tgt, refs)
            depth = 1 / disp[0]
            l1 = LF.photometric_reconstruction_loss(tgt, refs, K, Kinv, depth, None, pose, wssim=0)
            l3 = LF.smooth_loss(depth)
            scope.park_weight_gradients()
            (l1 + 0.1 * l3).backward()
            ops.wgrad_queue.flush()
            ops.wgrad_reduces.flush()
    finally:
        ops.packs.reset()
    LF.check_finite()
    return [t.detach().clone() for t in list(disp) + [pose, l1, l3, opt.flat_g]], log.calls


def trace_layers(dev):
    """-> (tensors, {name: calls in group spelling}) of the per-layer workloads"""
    tensors, calls = [], {}
    for name, kw in ALT_NETS:
        t, c = trace_alt(dev, name, kw)
        tensors += t
        calls[name] = group_spelling(c)
    t, c = trace_config1(dev)
    calls["config1"] = group_spelling(c)
    return tensors + t, calls


def plain(calls):
    """what json.load gives back for calls (float32 scalars as Python floats, tuples as lists)"""
    return json.loads(json.dumps(calls, default=float))


def load_fixture():
    with gzip.open(FIXTURE, "rt") as f:
        return json.load(f)


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from hipemu.emu import emulated_engine
    bits = sys.argv[sys.argv.index("--bits") + 1] if "--bits" in sys.argv else None
    out = FIXTURE if "--out" not in sys.argv else sys.argv[sys.argv.index("--out") + 1]
    with emulated_engine():
        tensors, fix = [], {}
        for name in TAPE_NETS:
            t, c = trace_tape("cpu", name)
            tensors += t
            fix["tape." + name] = plain(c)
        t, c = trace_step("cpu")
        tensors += t
        fix["step"] = plain(c)
        t, layers = trace_layers("cpu")
        tensors += t
        for k, c in layers.items():
            fix["layers." + k] = plain(c)
    with open(out, "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:      # (no name, no time: same bytes every time)
        f.write(("{\n" + ",\n".join('"%s": [\n%s\n]' % (k, ",\n".join(json.dumps(c, separators=(",", ":")) for c in v))
                                   for k, v in fix.items()) + "\n}\n").encode())
    print("wrote %s (%s calls)" % (out, {k: len(v) for k, v in fix.items()}))
    if bits:
        torch.save(tensors, bits)
        print("saved %d tensors to %s" % (len(tensors), bits))
