#!/usr/bin/env python
"""Headline benchmark: train images/sec of the Competitive-Collaboration step (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W
    (N > 1: launched by torch.distributed.run, one rank per GPU, RCCL gradient all-reduce)

One "step" = one full CC training step (train.py:445-568: DispResNet6 + PoseNetB6 + MaskNet6 + Back2Future
forward, 6-scale losses, backward, gradient all-reduce, Adam) on a synthetic per-GPU mini-batch of 4 five-frame
832x256 samples already resident in HBM.  value = N * 4 * K / time (whole-job images/sec, weak scaling).

A plain run sets up, warms up, times the K steps and prints the line.  --dump-outputs DIR also writes what the last timed step
computed (dump_outputs below).  Everything that takes runs of its own -- the objects below, the bench-time parity gate against
the CPU baseline, and at N > 1 the standalone and exposed communication figures -- runs only with --full.

Extra objects on the JSON line (--full):
  roofline      the dominant DEVICE kernel (the fp32 MFMA implicit-GEMM convolution with the largest share of the step):
                algorithmic FLOPs of its launches in one instrumented step / their durations -- HIP events recorded by the
                library around the kernel launch itself (cc_timing_*) -- against the 157.3 TFLOP/s fp32 MFMA peak; traffic =
                HBM bytes per launch of that kernel from the committed rocprofv3 PMC passes (profiles/pmc_traffic.json)
  kernels       the same for each C-ABI entry point (conv: TFLOP/s; warp/SSIM: algorithmic GB/s vs 8 TB/s HBM)
  cpu_baseline  the oracle (CPU port of the reference path, oracle/step.py) timed on this box's host cores
                (rank 0, N=1 only, bounded sample)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# The legacy STAGED data-parallel form (--pipeline staged with CC_NET_STREAMS=0) runs the HIP runtime with AMD_DIRECT_DISPATCH=0 -- set
# before the runtime is loaded.  With direct dispatch (the default) a stream-wait on ANOTHER stream's event -- what work.wait() of an
# asynchronous process-group collective is -- blocks the calling thread until that event has completed; the host then enqueues the
# optimizer launch and the next hipGraph replay with an idle GPU: measured +0.6 ms per step (profiles/r03_ab_round3.txt, r3z).  A
# graph with parallel branches pays +1.35 ms per replay for the setting (profiles/r05_ab_round5.txt), so it is applied to that form
# only.  The default form (round 6, per-network pipelines) has no host-side wait at all: its collectives are nodes of the graph.
if (int(os.environ.get("WORLD_SIZE", "1")) > 1 or os.environ.get("CC_FORCE_COMM", "0") == "1") and os.environ.get("CC_NET_STREAMS") == "0" \
        and "staged" in " ".join(sys.argv):
    os.environ.setdefault("AMD_DIRECT_DISPATCH", "0")

import torch                      # noqa: E402
import torch.distributed as dist  # noqa: E402

PEAK_MFMA_F32 = 157.3   # TFLOP/s, /opt/skills/guides/MI355X_MICROARCH.md
PEAK_HBM = 8000.0       # GB/s


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=4, help="per-GPU mini-batch")
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--width", type=int, default=832)
    ap.add_argument("--config", default="c3", choices=["c2", "c3"],
                    help="c3 = full CC (BASELINE configs[2], the metric's config); c2 = DispResNet6+PoseNetB6 only")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--elide-occ", action="store_true",
                    help="NOT the default metric: skip Back2Future's occlusion decoders, whose output train.py:463 discards "
                         "(SURVEY.md 8a D1); reported separately in DESIGN.md")
    ap.add_argument("--freeze", action="store_true",
                    help="README.md:59-65 training variant --fix-masknet --fix-flownet (train.py:332-346): all four nets run "
                         "forward, only DispResNet6 + PoseNetB6 are trained (227 MB gradient bucket); reported beside the metric")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check what the headline figure does not need: CPU baseline + parity gate, per-kernel "
                         "timing and roofline, and at N > 1 the standalone / exposed communication figures")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the losses, a seeded sample of the parameters and gradients, and the module buffers after the "
                         "last timed step as DIR/<name>.npy (float32 / float64).  In the library's default config.deterministic "
                         "mode the same arguments give the same arrays bit for bit -- at N > 1 only with an explicit --pipeline: "
                         "'auto' chooses the form by timing")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="(--full) skip the CPU baseline and the parity gate")
    ap.add_argument("--no-kernel-timing", action="store_true", help="(--full) skip the per-kernel timing and the roofline")
    ap.add_argument("--pipeline", choices=("auto", "per_network", "post", "staged"), default="auto",
                    help="per_network: every network's gradient all-reduce -> Adam segment -> weight images at the end of ITS "
                         "backward pass, on its own stream inside the one hipGraph; post: round 5 (one graph, two process-group "
                         "all-reduces behind it); staged: rounds 3-4 (two graphs, the first all-reduce between them); auto (default): "
                         "per_network -- and at N > 1, where no form has ever been measured on more than one GPU: the region is timed in "
                         "the post form first, then per_network runs a few untimed steps under a watchdog (CC_FORM_WATCHDOG_S, 240 s) and, "
                         "if faster, the region again; recorded in comm.form_selection.  If those steps never come back the watchdog "
                         "prints the post form's line and ends the run")
    ap.add_argument("--cpu-steps", type=int, default=3, help="timed CPU steps after one warm-up (median is reported)")
    ap.add_argument("--cpu-threads", type=int, default=0,
                    help="0 = min(usable threads (affinity / cgroup quota), 64): with all 256 hardware threads of the GPU box the "
                         "first oracle step did not finish in 13 min (round 2), with 64 threads a step takes ~8 s")
    ap.add_argument("--cpu-timeout", type=float, default=240.0, help="wall-clock bound of the CPU baseline leg (seconds)")
    ap.add_argument("--cpu-baseline-child", default=None, help=argparse.SUPPRESS)
    return ap.parse_args()


def self_launch(args):
    """`python bench.py --gpus N` outside a launcher: re-exec under torch.distributed.run, one rank per GPU (the driver's
    own command line for N > 1), and pass the ranks' output through."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    log("self-launch: " + " ".join(cmd))
    sys.exit(subprocess.call(cmd, env=env))


# ----------------------------------------------------------------------------- per-call instrumentation
def _px(args, names, *keys):
    d = dict(zip(names, args))
    r = 1
    for k in keys:
        r *= d[k]
    return r


WORK = {   # entry point -> (kind, fn(args dict) -> algorithmic flops or bytes)
    "cc_repack_table": ("byte", lambda d: 0.0),
    "cc_wgrad_reduce_table": ("byte", lambda d: 0.0),
    "cc_conv2d_fwd": ("flop", lambda d: 2.0 * d["B"] * d["OH"] * d["OW"] * d["Cout"] * d["Cin"] * d["R"] * d["S"]),
    "cc_conv2d_dgrad": ("flop", lambda d: 2.0 * d["B"] * d["OH"] * d["OW"] * d["K"] * d["C"] * d["R"] * d["S"]),
    "cc_conv2d_wgrad": ("flop", lambda d: 2.0 * d["B"] * d["AH"] * d["AW"] * d["M"] * d["Cin"] * d["R"] * d["S"]),
    # group forms: G same-shaped problems per launch
    "cc_conv2d_fwd_group": ("flop", lambda d: 2.0 * d["G"] * d["B"] * d["OH"] * d["OW"] * d["Cout"] * d["Cin"] * d["R"] * d["S"]),
    "cc_conv2d_dgrad_group": ("flop", lambda d: 2.0 * d["G"] * d["B"] * d["OH"] * d["OW"] * d["K"] * d["C"] * d["R"] * d["S"]),
    "cc_conv2d_wgrad_group": ("flop", lambda d: 2.0 * d["G"] * d["B"] * d["AH"] * d["AW"] * d["M"] * d["Cin"] * d["R"] * d["S"]),
    # n groups of different shapes in one call (the end-of-stage flush of the weight-gradient queue): desc_host = n x 32 longs
    "cc_conv2d_wgrad_list": ("flop", lambda d: wgrad_list_flops(d)),
    # algorithmic bytes per pixel (SURVEY.md 8d conventions: each distinct tensor argument once, fp32)
    "cc_inverse_warp_fwd": ("byte", lambda d: 28.0 * d["B"] * d["H"] * d["W"]),
    "cc_inverse_warp_bwd": ("byte", lambda d: 32.0 * d["B"] * d["H"] * d["W"]),
    "cc_flow_warp_fwd": ("byte", lambda d: 32.0 * d["B"] * d["H"] * d["W"]),
    "cc_flow_warp_bwd": ("byte", lambda d: 40.0 * d["B"] * d["H"] * d["W"]),
    "cc_pose2flow_fwd": ("byte", lambda d: 12.0 * d["B"] * d["H"] * d["W"]),
    # fused photometric body: reads tgt, warped (24) + two masks (8); with gradients writes 4 adjoint maps (48) + gmask (4)
    "cc_ssim_photo_fwd": ("byte", lambda d: (32.0 + (52.0 if d["want_grad"] else 0.0)) * d["B"] * d["H"] * d["W"]),
    # adjoint: reads 4 maps + tgt + warped (72), writes gwarped (12)
    "cc_ssim_photo_bwd": ("byte", lambda d: 84.0 * d["B"] * d["H"] * d["W"]),
    "cc_ssim_err_fwd": ("byte", lambda d: 32.0 * d["B"] * d["H"] * d["W"]),
    "cc_adam_step": ("byte", lambda d: 28.0 * d["n"]),
    # job-table forms: one launch = every (scale, reference frame) term of a loss; bytes/pixel as above, summed over the jobs
    "cc_inverse_warp_fwd_jobs": ("byte", lambda d: 28.0 * d["B"] * job_pixels(d)),
    "cc_inverse_warp_bwd_jobs": ("byte", lambda d: 32.0 * d["B"] * job_pixels(d)),
    "cc_flow_warp_fwd_jobs": ("byte", lambda d: 32.0 * d["B"] * job_pixels(d)),
    "cc_flow_warp_bwd_jobs": ("byte", lambda d: 40.0 * d["B"] * job_pixels(d)),
    "cc_pose2flow_fwd_jobs": ("byte", lambda d: 12.0 * d["B"] * job_pixels(d)),
    "cc_ssim_photo_fwd_jobs": ("byte", lambda d: (32.0 + (52.0 if d["want_grad"] else 0.0)) * d["B"] * job_pixels(d)),
    "cc_ssim_photo_bwd_jobs": ("byte", lambda d: 84.0 * d["B"] * job_pixels(d)),
    "cc_ssim_err_fwd_jobs": ("byte", lambda d: 32.0 * d["B"] * job_pixels(d)),
}


def wgrad_list_flops(d):
    """2 * MACs over the groups of a cc_conv2d_wgrad_list call (host records {G, a[4], x[4], gw[4], ws, B, M, AH, AW, a_bs, Cin,
    IH, IW, x_bs, R, S, ...} of 32 longs each, include/ccengine.h)."""
    import ctypes
    n = d["n"]
    arr = (ctypes.c_long * (32 * n)).from_address(d["desc_host"])
    tot = 0.0
    for i in range(n):
        r = arr[32 * i:32 * i + 32]
        tot += 2.0 * r[0] * r[14] * r[16] * r[17] * r[15] * r[19] * r[23] * r[24]
    return tot


def job_pixels(d):
    """sum of H*W over the jobs of a *_jobs call (the host job table: njobs x {8 slots, H, W} longs)."""
    import ctypes
    n = d["njobs"]
    arr = (ctypes.c_long * (10 * n)).from_address(d["jobs"])
    return float(sum(arr[10 * j + 8] * arr[10 * j + 9] for j in range(n)))


def call_group_of(name, d):
    """Label of a conv call group: the C-ABI entry point + the layer class (taps, stride, group size).  The device kernels behind
    a group are named by the library itself (tools build: cc_timing_collect -> `by_kernel`); nothing is inferred here."""
    if "R" not in d:
        return name
    r, s_, st = d.get("R"), d.get("S"), d.get("stride", d.get("si"))
    g = d.get("G", 1)
    return "%s %sx%s s%s%s" % (name, r, s_, st, " xG" if (g or 1) > 1 else "")


def algorithmic_bytes(name, d):
    """fp32 bytes of each distinct tensor argument once (input, weights, output) for one conv call."""
    if name == "cc_conv2d_wgrad_list":
        return 0.0
    if name.endswith("_group"):
        return d["G"] * algorithmic_bytes(name[:-6], d)
    if name == "cc_conv2d_fwd":
        return 4.0 * (d["B"] * d["Cin"] * d["IH"] * d["IW"] + d["Cout"] * d["Cin"] * d["R"] * d["S"] + d["B"] * d["Cout"] * d["OH"] * d["OW"])
    if name == "cc_conv2d_dgrad":
        return 4.0 * (d["B"] * d["K"] * d["OH"] * d["OW"] + d["K"] * d["C"] * d["R"] * d["S"] + d["B"] * d["C"] * d["IH"] * d["IW"])
    if name == "cc_conv2d_wgrad":
        return 4.0 * (d["B"] * d["M"] * d["AH"] * d["AW"] + d["B"] * d["Cin"] * d["IH"] * d["IW"] + d["M"] * d["Cin"] * d["R"] * d["S"])
    return 0.0


class CallTimer:
    """Brackets selected C-ABI calls with HIP events on the launch stream (torch's current stream)."""

    def __init__(self, eng):
        self.eng = eng
        self.records = []
        self.by_kernel = []
        self._orig = eng.call

    def __enter__(self):
        def call(name, *args):
            real = name
            if name == "cc_conv2d_wgrad_group_defer":      # same launch, its reduction parked (cc_wgrad_reduce_table)
                name = "cc_conv2d_wgrad_group"
            if name == "cc_conv2d_dgrad_group_add":        # same launch, further gradient contributions summed in its epilogue
                name = "cc_conv2d_dgrad_group"
            if name in WORK:
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                r = self._orig(real, *args)
                e.record()
                d = dict(zip(self.eng.sigs[real][2], args))
                if name.startswith("cc_conv2d_"):
                    self.by_kernel.append((call_group_of(name, d), WORK[name][1](d), algorithmic_bytes(name, d), s, e))
                self.records.append((name, WORK[name][1](d), s, e, {k: v for k, v in d.items() if isinstance(v, int) and k not in ("x_bs", "y_bs", "res_bs", "a_bs", "gy_bs", "gx_bs")}))
                return r
            return self._orig(name, *args)
        self.eng.call = call
        return self

    def __exit__(self, *a):
        self.eng.call = self._orig

    def kernel_groups(self):
        """-> {call group: {launches, ms, gflop, bytes}} over the conv calls (one call = its main kernel launch(es) plus the
        epilogue / reduction launches it issues)."""
        torch.cuda.synchronize()
        g = {}
        for kn, fl, by, s, e in self.by_kernel:
            a = g.setdefault(kn, {"launches": 0, "ms": 0.0, "gflop": 0.0, "bytes": 0.0})
            a["launches"] += 1
            a["ms"] += s.elapsed_time(e)
            a["gflop"] += fl / 1e9
            a["bytes"] += by
        return g

    def summary(self):
        torch.cuda.synchronize()
        agg = {}
        detail = {}
        for name, work, s, e, shp in self.records:
            key = name + " " + " ".join("%s=%s" % kv for kv in sorted(shp.items()))
            dd = detail.setdefault(key, [0, 0.0, 0.0])
            dd[0] += 1
            dd[1] += work
            dd[2] += s.elapsed_time(e)
        if os.environ.get("CC_BENCH_DETAIL"):
            with open(os.environ["CC_BENCH_DETAIL"], "w") as f:
                for key, (n, work, ms) in sorted(detail.items(), key=lambda kv: -kv[1][2]):
                    f.write("%8.3f ms  n=%3d  %7.2f G  %6.1f rate  %s\n" % (ms, n, work / 1e9, work / ms / 1e9 if ms > 0 else 0, key))
        for name, work, s, e, shp in self.records:
            a = agg.setdefault(name, [0, 0.0, 0.0])
            a[0] += 1
            a[1] += work
            a[2] += s.elapsed_time(e)
        out = {}
        for name, (n, work, ms) in agg.items():
            kind = WORK[name][0]
            rate = work / (ms * 1e-3) / (1e12 if kind == "flop" else 1e9) if ms > 0 else 0.0
            out[name] = {"calls": n, "ms": round(ms, 4), "avg_us": round(1e3 * ms / n, 2),
                         ("tflops" if kind == "flop" else "gbps"): round(rate, 2),
                         "frac": round(rate / (PEAK_MFMA_F32 if kind == "flop" else PEAK_HBM), 4)}
        return out


def log(*a):
    print("[bench]", *a, file=sys.stderr, flush=True)


DUMP_SAMPLE = 1 << 22      # elements drawn from each of the parameter and gradient vectors: 2 x 16 MB of float32


def output_snapshot(tr, losses):
    """What a caller of the timed step holds after its last step, as host arrays: the loss terms (float64), the networks'
    trainable parameters and their gradients in chain order (float32; where there are more than DUMP_SAMPLE elements, the same
    fixed sample of both, drawn with seed 0 and sorted), and the module buffers (BatchNorm running statistics, float64).
    Taken right after the timed region, before any other step moves the weights.  -> {name: numpy array}"""
    import numpy as np
    torch.cuda.synchronize()
    out = {k: np.array(float(v), dtype=np.float64) for k, v in losses.items()}
    p, g = tr.opt.gather(tr.opt.flat_p), tr.opt.gather(tr.opt.flat_g)
    if p.numel() > DUMP_SAMPLE:
        idx = torch.unique(torch.randint(0, p.numel(), (DUMP_SAMPLE,), generator=torch.Generator().manual_seed(0)))
        p, g = p[idx.to(p.device)], g[idx.to(g.device)]
    out["params"], out["grads"] = p.cpu().numpy(), g.cpu().numpy()
    bufs = [b.detach().reshape(-1).double() for n_ in tr.nets if n_ is not None for b in n_.buffers()]
    if bufs:
        out["buffers"] = torch.cat(bufs).cpu().numpy()
    return out


def dump_outputs(d, arrays):
    import numpy as np
    os.makedirs(d, exist_ok=True)
    for k, v in arrays.items():
        np.save(os.path.join(d, k + ".npy"), v)
    log("wrote %d arrays (%.1f MB) to %s" % (len(arrays), sum(v.nbytes for v in arrays.values()) / 1e6, d))


def pmc_traffic(kernel):
    """HBM bytes per launch of `kernel` from the committed rocprofv3 PMC passes of this same command
    (profiles/pmc_traffic.json, written by tools/pmc_traffic.py: (2*FETCH_SIZE + WRITE_SIZE) KiB per dispatch, the
    gfx950 FETCH_SIZE correction of MI355X_MICROARCH.md).  bench.py cannot run the profiler on itself."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "pmc_traffic.json")
    try:
        with open(path) as f:
            t = json.load(f)
        from cc_amd import _lib
        have = int(_lib.engine().call("cc_version"))
        if int(t.get("cc_version", -1)) != have:
            return None, "profiles/pmc_traffic.json is stale (kernels %s, library %s): rerun tools/gpu_pmc2.sh" % (
                t.get("cc_version"), have)
        name = kernel.replace(" xG", "").split("+")[0]
        ent = t["kernels"].get(name)
        if ent:
            return round(ent["hbm_bytes_per_launch"]), "profiles/pmc_traffic.json (%s)" % t.get("command", "")
        # the timing registry names a kernel by its leading template arguments (k_wino_f2x3<0> = every epilogue variant
        # k_wino_f2x3<0, *, *>): launch-weighted mean over the variants
        if name.endswith(">"):
            var = [v for k, v in t["kernels"].items() if k.startswith(name[:-1] + ",")]
            n_ = sum(v["launches"] for v in var)
            if n_:
                return (round(sum(v["hbm_bytes_per_launch"] * v["launches"] for v in var) / n_),
                        "profiles/pmc_traffic.json, launch-weighted mean of %d template variants (%s)" % (len(var), t.get("command", "")))
    except (OSError, ValueError, KeyError):
        pass
    return None, None


def usable_cpus():
    """Threads this process may actually run on: scheduler affinity, capped by a cgroup CPU quota when there is one
    (os.cpu_count() reports the whole machine inside a container; a thread pool sized by it spin-waits itself to a halt)."""
    try:
        n = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        n = os.cpu_count() or 1
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            with open(path) as f:
                parts = f.read().split()
            if path.endswith("cpu.max"):
                if parts[0] != "max":
                    n = min(n, max(1, int(float(parts[0]) / float(parts[1]))))
            else:
                q = int(parts[0])
                if q > 0:
                    with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as g:
                        n = min(n, max(1, q // int(g.read().split()[0])))
        except (OSError, ValueError, IndexError):
            pass
    return n


def cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for ln in f:
                if ln.startswith("model name"):
                    return ln.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(batch_cpu, init_sd, args):
    """The reference's own modules (oracle/_ref/ccref.zip: the unmodified files of SURVEY.md 8a packed by `make -C oracle` in the
    build container, loaded through oracle/ref_import.py's two shims) -- or, where that archive is missing, the oracle (the CPU
    port pinned bit-exact to the reference by tests/golden) -- on this box's host cores.  Reported beside the metric, never
    the target.  It starts from the SAME initial weights as the GPU run, so its first two steps double as the bench-time
    parity gate.  -> (baseline dict, [losses per step])"""
    from oracle import step as S
    from oracle import ref_import
    n = args.cpu_threads if args.cpu_threads > 0 else min(usable_cpus(), 64)
    torch.set_num_threads(n)
    impl, kind = None, "port"
    if ref_import.reference_available():
        try:
            impl = ref_import.load()
            kind = "reference"
        except Exception as e:                                   # noqa: BLE001 -- any import problem: fall back to the port
            log("reference modules unusable (%r): timing the CPU port instead" % (e,))
            impl = None
    if impl is not None:
        nets = S.build_nets("ref", impl, flow=(args.config == "c3"), mask=(args.config == "c3"))
    else:
        nets = S.build_nets("oracle", flow=(args.config == "c3"), mask=(args.config == "c3"))
    for m, sd in zip(nets, init_sd):
        if m is not None:
            m.load_state_dict(sd)
            m.train()
    if args.freeze:
        for m in nets[2:]:
            if m is not None:
                for p_ in m.parameters():
                    p_.requires_grad = False              # train.py:332-339
    cfg = S.StepConfig()
    opt = S.make_optimizer(nets, cfg)
    losses, times = [], []
    first = {}
    for i in range(1 + args.cpu_steps):
        t0 = time.time()
        if i == 0:      # (the untimed warm-up step also keeps d loss / d (network outputs) for the gradient pin, tools/grad_pin.py)
            l0, first["out_grads"] = S.cc_step_keep(nets, opt, batch_cpu, cfg, impl)
            losses.append(l0)
        else:
            losses.append(S.cc_step(nets, opt, batch_cpu, cfg, impl))
        times.append(time.time() - t0)
        log("cpu baseline step %d: %.1f s (%d threads)" % (i, times[-1], n))
        if i == 0:      # for the parity gate: gradient norms of the first step and the parameters after its Adam update
            first["grad_norm"] = [float(torch.sqrt(sum((p_.grad.double() ** 2).sum() for p_ in m.parameters()
                                                       if p_.requires_grad and p_.grad is not None)))
                                  for m in nets if m is not None and any(p_.requires_grad for p_ in m.parameters())]
            first["params"] = torch.cat([p_.detach().reshape(-1) for m in nets if m is not None
                                         for p_ in m.parameters() if p_.requires_grad]).clone()
            first["grads"] = torch.cat([(p_.grad if p_.grad is not None else torch.zeros_like(p_)).detach().reshape(-1)
                                        for m in nets if m is not None for p_ in m.parameters() if p_.requires_grad]).clone()
    if first.get("out_grads") is not None and not args.freeze:
        # for the gradient pin (tools/grad_pin.py, untimed): the exact (float64) parameter gradient of the same weights and output
        # gradients, and how far the reference's own fp32 gradient moves under 1e-7 input noise (its condition)
        try:
            from tools import grad_pin
            first["grads64"] = grad_pin.fp64_param_grads(init_sd, batch_cpu, first["out_grads"])
            first["cond"] = grad_pin.conditioning(init_sd, batch_cpu, first["out_grads"])
        except Exception as e:                                   # noqa: BLE001
            log("gradient pin: fp64 / conditioning pass failed (%r)" % (e,))
    timed = sorted(times[1:])
    dt = timed[len(timed) // 2] if timed else times[0]
    what = ("the reference's own inverse_warp / loss_functions / ssim / models files (oracle/_ref/ccref.zip, unmodified; two "
            "import shims: the absent spatial_correlation_sampler CUDA extension restated in torch, .cuda() a no-op) driven by "
            "oracle/step.py's mirror of train.py:445-568" if kind == "reference" else
            "oracle/step.py (the CPU port of train.py:445-568, pinned to the reference by tests/golden)")
    return {"value": round(batch_cpu[0].shape[0] / dt, 4), "unit": "images/s", "cores": n, "kind": kind,
            "cpu": cpu_model(), "host_threads": os.cpu_count(), "usable_threads": usable_cpus(),
            "sample": "median of %d full CC steps (fwd+bwd+Adam) after 1 warm-up, B=%d %dx%d, %s, torch %s, %d threads"
                      % (len(timed), batch_cpu[0].shape[0], batch_cpu[0].shape[3], batch_cpu[0].shape[2], what,
                         torch.__version__, n),
            "s_per_step": round(dt, 3), "s_per_step_all": [round(t, 3) for t in times]}, losses, first


def cpu_baseline_bounded(batch_cpu, init_sd, args):
    """Run cpu_baseline() in a child process with a wall-clock bound, so that a slow host can never eat the bench line.
    -> (baseline dict or {'value': None, 'note': ...}, [losses per step], {'grad_norm': [...], 'params': tensor} of the first step)"""
    import subprocess
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        inp, outp = os.path.join(td, "in.pt"), os.path.join(td, "out.json")
        torch.save({"batch": batch_cpu, "init_sd": init_sd}, inp)
        cmd = [sys.executable, os.path.abspath(__file__)] + sys.argv[1:] + ["--cpu-baseline-child", inp + "," + outp]
        env = dict(os.environ)
        env["HIP_VISIBLE_DEVICES"] = ""            # the child is a pure CPU process
        try:
            subprocess.run(cmd, env=env, timeout=args.cpu_timeout, check=True, stdout=sys.stderr)
            with open(outp) as f:
                r = json.load(f)
            first = {"grad_norm": r.get("grad_norm", [])}
            if os.path.isfile(outp + ".params.pt"):
                blob = torch.load(outp + ".params.pt")
                first["params"], first["grads"] = blob[0], blob[1]
                if len(blob) > 2:
                    first["out_grads"] = blob[2]
                if len(blob) > 4:
                    first["grads64"], first["cond"] = blob[3], blob[4]
            return r["baseline"], r["losses"], first
        except subprocess.TimeoutExpired:
            return {"value": None, "unit": "images/s", "kind": "port", "cpu": cpu_model(), "host_threads": os.cpu_count(),
                    "note": "CPU baseline leg exceeded --cpu-timeout %.0f s" % args.cpu_timeout}, [], {}
        except (subprocess.CalledProcessError, OSError, ValueError) as e:
            return {"value": None, "unit": "images/s", "kind": "port", "note": "CPU baseline leg failed: %r" % (e,)}, [], {}


def main():
    args = parse()
    if args.cpu_baseline_child:
        inp, outp = args.cpu_baseline_child.split(",")
        d = torch.load(inp)
        base, losses, first = cpu_baseline(d["batch"], d["init_sd"], args)
        if "params" in first:
            torch.save((first["params"], first["grads"], first.get("out_grads"), first.get("grads64"), first.get("cond")), outp + ".params.pt")
        with open(outp, "w") as f:
            json.dump({"baseline": base, "losses": losses, "grad_norm": first.get("grad_norm", [])}, f)
        return
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(args)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    assert torch.cuda.is_available(), "bench.py needs HIP devices (there is no CPU path)"
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    # CC_FORCE_COMM=1 on one GPU: a 1-rank RCCL group, so that the N > 1 code path (two graphs, segment all-reduces, the
    # communication record of the JSON line) can be exercised where only one GPU is available
    use_dist = world > 1 or os.environ.get("CC_FORCE_COMM", "0") == "1"
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group("nccl", rank=rank, world_size=world)     # nccl == RCCL on ROCm
    assert world == args.gpus, "launch with torch.distributed.run --nproc-per-node %d" % args.gpus

    from tools import ab_env
    ab_switches = ab_env.apply()            # CC_* A/B variables -> cc_amd.config.debug, BEFORE the first engine() call (library path);
    #                                         explicit: the package itself reads no environment variable
    from cc_amd import synthetic as syn, trainer as T, _lib, config as cc_config
    eng = _lib.engine()

    torch.manual_seed(0)                                             # train.py:152
    nets = T.build_nets(dev, flow=(args.config == "c3"), mask=(args.config == "c3"))
    cfg = T.StepConfig()
    if args.elide_occ and nets[3] is not None:
        nets[3].elide_occ = True
    if args.freeze:
        for n_ in nets[2:]:
            if n_ is not None:
                for p_ in n_.parameters():
                    p_.requires_grad = False                             # train.py:332-339
    want_cpu = args.full and rank == 0 and world == 1 and not args.no_cpu_baseline
    init_sd = [({k: v.detach().cpu().clone() for k, v in n_.state_dict().items()} if n_ is not None else None)
               for n_ in nets] if want_cpu else None
    B, H, W = args.batch, args.height, args.width
    batch_cpu = syn.sample(B, H, W, seed=1 + rank, smooth=3)
    batch = (batch_cpu[0].to(dev), [r.to(dev) for r in batch_cpu[1]], batch_cpu[2].to(dev), batch_cpu[3].to(dev))
    # measurement switches of the data-parallel step (tools/gpu_r3y.sh, gpu_r3z.sh): read HERE, by the measuring script -- the
    # product step (cc_amd/trainer.py) reads no environment variable
    if os.environ.get("CC_NO_HEAD_ACC", "0") == "1":                    # A/B: the loss terms return separate gradients, the engine adds them
        from cc_amd import loss_functions as _LF
        _LF.head_grads.enabled = False
    comm_debug = {"events": os.environ.get("CC_NO_COMM_EVENTS", "0") != "1"}
    if os.environ.get("CC_COMM_JOIN"):
        comm_debug["join"] = os.environ["CC_COMM_JOIN"]
    if os.environ.get("CC_COMM_PROBE"):
        comm_debug["probe"] = os.environ["CC_COMM_PROBE"]
    ab_env.assert_applied()
    pipe = ab_switches.get("pipeline", args.pipeline)
    # auto at N > 1: the step starts in round 5's "post" form (process-group all-reduce behind the graph: the conventional path), is
    # timed in it, and only then tries the per-network form under a watchdog (select_form below) -- a captured-RCCL form that has never
    # run on more than one GPU must not be able to cost the run its number
    select = pipe == "auto" and use_dist and (world > 1 or os.environ.get("CC_FORCE_FORM_SELECTION") == "1") and not args.no_graph
    tr = T.CCTrainer(nets, cfg, use_graph=not args.no_graph, comm_debug=comm_debug,
                     pipeline=("post" if select else "per_network") if pipe == "auto" else pipe)

    def sync():
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
            torch.cuda.synchronize()

    t_w = time.perf_counter()
    first_losses = []
    for i in range(args.warmup):
        losses = tr.step(batch)
        if rank == 0:
            torch.cuda.synchronize()
            if i < 2:
                first_losses.append({k: float(v) for k, v in losses.items()})
            if i == 0 and want_cpu:      # (parity gate) gradient norms of the first step, parameters after its update
                first_gn = [float(torch.sqrt(sum((p_.grad.double() ** 2).sum() for p_ in n_.parameters() if p_.requires_grad)))
                            for n_ in nets if n_ is not None and any(p_.requires_grad for p_ in n_.parameters())]
                first_params = tr.opt.gather(tr.opt.flat_p).detach().cpu().clone()       # (chain order, without the bucket's padding)
                first_grads = tr.opt.gather(tr.opt.flat_g).detach().cpu().clone()
            log("warm-up step %d done at %.1f s" % (i, time.perf_counter() - t_w))
    def timed_region():
        """EXACTLY args.steps steps between barrier + synchronize; per-step device time stamps: an event after every step on the
        compute stream (no host synchronisation inside the region).  -> (wall seconds of this rank, sorted per-step ms, last losses,
        output_snapshot of the last step or None)"""
        sync()
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
        t0_ = time.perf_counter()
        marks[0].record()
        for i in range(args.steps):
            ls_ = tr.step(batch)
            marks[i + 1].record()
        sync()
        dt_ = time.perf_counter() - t0_
        snap_ = output_snapshot(tr, ls_) if args.dump_outputs and rank == 0 else None
        return dt_, sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(args.steps)), ls_, snap_

    def max_over_ranks(x):
        if not use_dist:
            return float(x)
        t_ = torch.tensor([x], device=dev, dtype=torch.float64)
        dist.all_reduce(t_, op=dist.ReduceOp.MAX)
        return float(t_.item())

    def contract_line(dt_max, loss_, pipeline, extra_comm):
        """the driver's keys alone (the emergency line of the watchdog below; the full line is assembled at the end of main)"""
        return {"metric": "train images/sec (%dx%d, 5-frame sample, 6-scale CC step)" % (W, H),
                "value": round(B * world * args.steps / dt_max, 3), "unit": "images/s", "n_gpus": world, "steps": args.steps,
                "warmup": args.warmup, "ms_per_step": round(1e3 * dt_max / args.steps, 3), "higher_is_better": True,
                "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
                "config": {"workload": "full CC: DispResNet6+PoseNetB6+MaskNet6+Back2Future, all losses" if args.config == "c3"
                           else "DispResNet6+PoseNetB6, photometric+smoothness", "per_gpu_batch": B, "global_batch": B * world,
                           "height": H, "width": W, "scales": 6, "frames": 5, "parallelism": "dp%d" % world, "hipgraph": True,
                           "loss": round(float(loss_), 6), "pipeline": pipeline},
                "comm": extra_comm, "roofline": None}

    form_selection, first_region = None, None
    if select and tr.pipeline == "post":
        # No step form has been measured on more than one GPU (rounds 1-6: one GPU per gpurun call).  The "post" form is timed FIRST,
        # over the full region; then the per-network form (collectives INSIDE the replayed graph, cc_amd/rccl.py) runs a few untimed
        # steps under a watchdog, and if it is the faster one -- max over ranks -- the region is timed again in it.  Should those steps
        # not come back (captured collectives of three communicators on three graph branches: nothing says they cannot wedge on a
        # machine this code has never seen), every rank's watchdog ends its process after rank 0 has printed the line of the "post"
        # region -- the run keeps its number and says what happened.
        import threading
        dt_post, steps_post, losses_post, snap_post = timed_region()
        dt_post_max = max_over_ranks(dt_post)
        ms_post = 1e3 * dt_post_max / args.steps
        limit = float(os.environ.get("CC_FORM_WATCHDOG_S", "240"))
        disarm = threading.Event()

        def _watch():
            if disarm.wait(limit):
                return
            if rank == 0:
                sel = {"post_ms": round(ms_post, 3), "chosen": "post",
                       "per_network": "its first steps did not finish within %.0f s: watchdog ended the run on the post form's line" % limit}
                log("form selection: the per-network form did not come back within %.0f s -- printing the post form's line" % limit)
                print(json.dumps(contract_line(dt_post_max, losses_post["loss"], "post", {"form_selection": sel})), flush=True)
            else:
                time.sleep(2.0)
            os._exit(0)
        threading.Thread(target=_watch, daemon=True).start()
        ms_pn, why = None, None
        try:
            tr.switch_pipeline("per_network")
            for _ in range(3):
                tr.step(batch)
            sync()
            if tr.pipeline == "per_network":          # (the trainer falls back to "post" by itself when the capture is refused)
                ta = time.perf_counter()
                for _ in range(6):
                    tr.step(batch)
                sync()
                ms_pn = max_over_ranks((time.perf_counter() - ta) / 6 * 1e3)
            else:
                why = "capture or communicator set-up refused (see stderr)"
        except Exception as e:      # noqa: BLE001 -- an RCCL error code: stay on the form that works
            why = repr(e)
        # every rank must take the same branch: a rank that failed alone would leave the others in a collective
        fl = torch.tensor([0.0 if ms_pn is not None else 1.0], device=dev, dtype=torch.float64)
        dist.all_reduce(fl, op=dist.ReduceOp.MAX)
        if float(fl.item()) > 0:
            ms_pn = None
        # ... and the per-network form with DispResNet6's segment handed over in chunks while its backward pass still runs
        # (config.grad_chunks: slower on one GPU, where it hides nothing; data-parallel it starts the one exchange that no other
        # network's backward pass covers early) -- a third candidate, under the same watchdog
        ms_ch = None
        if ms_pn is not None:
            try:
                tr.set_grad_chunks(True)
                for _ in range(3):
                    tr.step(batch)
                sync()
                ta = time.perf_counter()
                for _ in range(6):
                    tr.step(batch)
                sync()
                ms_ch = max_over_ranks((time.perf_counter() - ta) / 6 * 1e3)
            except Exception as e:      # noqa: BLE001
                why = "with gradient chunks: " + repr(e)
            fl = torch.tensor([0.0 if ms_ch is not None else 1.0], device=dev, dtype=torch.float64)
            dist.all_reduce(fl, op=dist.ReduceOp.MAX)
            if float(fl.item()) > 0:
                ms_ch = None
        cands = [("post", ms_post)] + ([("per_network", ms_pn)] if ms_pn is not None else []) + \
                ([("per_network+grad_chunks", ms_ch)] if ms_ch is not None else [])
        chosen_full = min(cands, key=lambda kv: kv[1])[0]
        chosen = "post" if chosen_full == "post" else "per_network"
        tr.grad_chunks = chosen_full == "per_network+grad_chunks"
        tr.switch_pipeline(chosen)          # (drops the captured graph: the next step captures the chosen form)
        for _ in range(3):
            tr.step(batch)
        sync()
        form_selection = {"post_ms": round(ms_post, 3), "per_network_ms": round(ms_pn, 3) if ms_pn is not None else None,
                          "per_network_grad_chunks_ms": round(ms_ch, 3) if ms_ch is not None else None,
                          "chosen": chosen_full, "per_network_failed": why,
                          "how": "post: the full timed region; per_network: 6 replayed steps after 3 untimed ones under a %.0f s watchdog, "
                                 "max over ranks; the chosen form runs the reported region" % limit}
        log("form selection: post %.2f ms, per_network %s, with gradient chunks %s -> %s"
            % (ms_post, ("%.2f ms" % ms_pn) if ms_pn is not None else "failed", ("%.2f ms" % ms_ch) if ms_ch is not None else "-", chosen_full))
        if chosen == "post":
            disarm.set()
            first_region = (dt_post, steps_post, losses_post, snap_post)
    if use_dist and args.full:
        tr.calibrate_comm()                 # each segment's all-reduce alone (outside the timed region)
    dt, per_step, losses, snap = first_region if first_region is not None else timed_region()
    if snap is not None:
        dump_outputs(args.dump_outputs, snap)
    if select and form_selection is not None and form_selection["chosen"] != "post":
        disarm.set()

    def pct(q):
        return round(per_step[min(len(per_step) - 1, int(q * len(per_step)))], 3)
    step_ms = {"median": pct(0.5), "p10": pct(0.1), "p90": pct(0.9), "min": round(per_step[0], 3), "max": round(per_step[-1], 3),
               "source": "HIP events after every step on the compute stream; `ms_per_step` is the wall-clock mean of the region"}
    comm = tr.comm_stats() if use_dist else None
    if comm is not None and form_selection is not None:
        comm["form_selection"] = form_selection
    rank_losses = None
    if use_dist:
        lt = torch.tensor([float(losses["loss"]), step_ms["median"]], device=dev, dtype=torch.float64)
        allv = [torch.zeros_like(lt) for _ in range(world)]
        dist.all_gather(allv, lt)
        rank_losses = [round(float(v[0].item()), 6) for v in allv]
        if comm is not None:
            # what the first real multi-GPU run needs to explain itself: every rank's own median step time (a straggler shows here,
            # the MAX is the metric), and backward stage B with the 227 MB all-reduce in flight against the same stage with the
            # collectives skipped (RCCL's workgroups take CUs from the MFMA kernels; measured AFTER the timed region and the parity
            # gate -- the ranks' weights diverge in those few steps, nothing is reported from them but the stage time)
            comm["rank_step_ms_median"] = [round(float(v[1].item()), 3) for v in allv]
            comm["stage_b_ms"] = {"with_allreduce_in_flight": tr.stage_b_ms()} if tr.graph_b is not None else None
    if use_dist:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    loss_val = float(losses["loss"])
    if rank == 0:
        log("timed %d steps: %.2f ms/step, loss %.6f" % (args.steps, 1e3 * dt / args.steps, loss_val))
    tr.check_finite()
    if args.full and use_dist and comm is not None and tr.graph_b is not None and not tr.opt.comm_probe:
        # backward stage B with the collectives skipped (see comm.stage_b_ms above): a few untimed steps
        tr.opt.comm_probe, tr.stage_b_events = "skip", []
        for _ in range(6):
            tr.step(batch)
        sync()
        comm["stage_b_ms"]["collectives_skipped"] = tr.stage_b_ms()
        tr.opt.comm_probe = ""

    if args.full and use_dist and comm is not None and tr.pipeline == "per_network" and not tr.opt.comm_probe and not args.no_graph:
        # EXPOSED communication of the per-network form: its collectives are nodes of the replayed graph (no event can bracket them),
        # so the same step is captured once more with the collectives skipped and timed over a few steps AFTER the timed region and the
        # parity gate (the ranks' weights diverge in those steps; nothing else is reported from them).  exposed = with - without.
        n_ab = max(5, min(args.steps, 20))
        tr.opt.comm_probe, tr.graph = "skip", None

        def _time_steps():
            for _ in range(3):
                tr.step(batch)
            sync()
            ta = time.perf_counter()
            for _ in range(n_ab):
                tr.step(batch)
            sync()
            t_ = torch.tensor([(time.perf_counter() - ta) / n_ab * 1e3], device=dev, dtype=torch.float64)
            dist.all_reduce(t_, op=dist.ReduceOp.MAX)
            return float(t_.item())
        ms_skip = _time_steps()
        tr.opt.comm_probe, tr.graph = "", None
        ms_with = _time_steps()
        comm["step_ms_with_collectives"] = round(ms_with, 3)
        comm["step_ms_collectives_skipped"] = round(ms_skip, 3)
        comm["exposed_ms_total"] = round(ms_with - ms_skip, 3)
        comm["exposed_how"] = ("max-over-ranks wall-clock mean of %d replayed steps with the collectives in the graph minus the same with "
                               "them skipped (re-captured; measured back to back after the timed region)" % n_ab)

    kernels, roof = None, None
    if args.full and not args.no_kernel_timing:
        tr_e = tr
        tr_e.use_graph = False
        # Per-kernel and per-call durations are taken with the networks' side streams OFF: a kernel that shares the chip with another
        # stream's kernel takes longer without being a worse kernel, and HIP-event brackets around overlapping launches do not add up.
        # The timed region above ran with them on (config.net_streams); the dominant kernel's rate as it runs THERE is reported beside
        # the isolated one (roofline.with_network_streams).
        saved_streams = tr_e.net_streams
        tr_e.net_streams = None
        with CallTimer(eng) as ct:
            tr_e.step(batch)
        kernels = ct.summary()
        groups = ct.kernel_groups()
        convs = {k: v for k, v in kernels.items() if "tflops" in v}
        # per-device-kernel durations: HIP events around the kernel launch itself, recorded inside the library (cc_timing_*),
        # so that the roofline line names a kernel of the rocprofv3 summary and quotes ITS duration (not the C-ABI call's,
        # which for split-K layers also contains the epilogue launch)
        import ctypes
        from cc_amd import build as _build
        dev_lines = []
        try:
            tools_lib = _build.TOOLS_OUT if os.path.isfile(_build.TOOLS_OUT) else _build.build_tools()
            # the timing registry lives in the TOOLS build of the library only (same sources, -DCC_TOOLS); the product library that
            # ran the timed region above keeps no state
            with _lib.use_library(tools_lib) as teng:
                assert teng.fn["cc_is_tools_build"]() == 1
                tr_e.step(batch)                       # first launches from this library image (code object load) stay untimed
                torch.cuda.synchronize()
                teng.call("cc_timing_enable", 1)
                tr_e.step(batch)
                torch.cuda.synchronize()
                buf = ctypes.create_string_buffer(1 << 18)
                nchar = teng.fn["cc_timing_collect"](ctypes.addressof(buf), 1 << 18)
                dev_lines = buf.raw[:nchar].decode().splitlines()
                if os.environ.get("CC_TIMING_DUMP"):      # tools/layer_rates.py: the per-shape table (CC_TIMING_DETAIL=1)
                    with open(os.environ["CC_TIMING_DUMP"], "w") as f:
                        f.write("\n".join(dev_lines) + "\n")
                dev_lines_conc = []
                if saved_streams:
                    tr_e.net_streams = saved_streams
                    teng.call("cc_timing_enable", 0)
                    tr_e.step(batch)
                    torch.cuda.synchronize()
                    teng.call("cc_timing_enable", 1)
                    tr_e.step(batch)
                    torch.cuda.synchronize()
                    nchar = teng.fn["cc_timing_collect"](ctypes.addressof(buf), 1 << 18)
                    dev_lines_conc = buf.raw[:nchar].decode().splitlines()
        except (RuntimeError, OSError, AssertionError) as e:
            log("tools build unavailable (%r): no per-device-kernel timing" % (e,))
            dev_lines_conc = []
        tr_e.net_streams = saved_streams
        dev_k = {}
        for ln in dev_lines:
            nm, n_, ms_, gf_ = ln.split("\t")
            dev_k[nm] = {"launches": int(n_), "ms": float(ms_), "gflop": float(gf_)}
        if dev_k:
            # the dominant kernel = the device kernel with the largest share of the step
            kn, a = max(dev_k.items(), key=lambda kv: kv[1]["ms"])
            ach = a["gflop"] / a["ms"] if a["ms"] > 0 else 0.0                       # GFLOP / ms = TFLOP/s
            tot_ms = sum(v["ms"] for v in convs.values())
            tot_fl = sum(v["tflops"] * v["ms"] for v in convs.values())
            fam = tot_fl / tot_ms if tot_ms > 0 else 0.0
            traffic, src = pmc_traffic(kn)
            eager = {k: {"launches": v["launches"], "ms": round(v["ms"], 3),
                         "tflops": round(v["gflop"] / v["ms"], 2) if v["ms"] > 0 else 0.0}
                     for k, v in sorted(groups.items(), key=lambda kv: -kv[1]["ms"])[:6]} if groups else None
            wino = kn.startswith("k_wino")        # Winograd kernels: the numerator is the MFMA FLOPs they EXECUTE (16 multiply-adds per
            #                                         2x2 tile and channel pair; the direct form of the same layers has 36)

            def _k(k, v):
                r = {"launches": v["launches"], "ms": round(v["ms"], 3), "tflops": round(v["gflop"] / v["ms"], 2) if v["ms"] > 0 else 0.0}
                if k.startswith("k_wino"):
                    r["direct_equivalent_tflops"] = round(2.25 * r["tflops"], 2)
                return r
            mfma_k = {k: v for k, v in dev_k.items() if v["gflop"] > 0}
            ex_ms, ex_gf = sum(v["ms"] for v in mfma_k.values()), sum(v["gflop"] for v in mfma_k.values())
            # "library": the per-kernel durations come from the TOOLS build of the same sources (timing registry compiled in, default
            # thresholds); the timed region above ran on the product library
            conc = None
            for ln in dev_lines_conc:
                nm, n_, ms_, gf_ = ln.split("\t")
                if nm == kn and float(ms_) > 0:
                    conc = {"achieved": round(float(gf_) / float(ms_), 2), "frac": round(float(gf_) / float(ms_) / PEAK_MFMA_F32, 4),
                            "avg_launch_us": round(1e3 * float(ms_) / int(n_), 2),
                            "what": "the same kernel in an eager step with the networks on their side streams: its launches share the "
                                    "chip with the other streams' kernels"}
            roof = {"library": "tools", "measured_with": "network side streams off (kernels one after the other)",
                    "with_network_streams": conc, "bound": "mfma", "kernel": kn, "achieved": round(ach, 2), "peak": PEAK_MFMA_F32, "unit": "TFLOP/s",
                    "frac": round(ach / PEAK_MFMA_F32, 4), "traffic": traffic, "traffic_source": src,
                    "launches": a["launches"], "avg_launch_us": round(1e3 * a["ms"] / a["launches"], 2),
                    "timing": "HIP events around the kernel launch on its stream (cc_timing_enable / cc_timing_collect), one "
                              "eager step; all launches of this device kernel in the step (grouped, split-K and plain)",
                    "algorithmic_gflop_per_launch": round(a["gflop"] / a["launches"], 3),
                    "flops": ("MFMA FLOPs executed by the Winograd F(2x2, 3x3) kernel = 4/9 of the direct form's 2*MACs of the same layers"
                              if wino else "2*MACs of the layers"),
                    "direct_equivalent_tflops": round(2.25 * ach, 2) if wino else None,
                    "ms_per_step": round(a["ms"], 3),
                    "conv_family": {"achieved": round(fam, 2), "frac": round(fam / PEAK_MFMA_F32, 4),
                                    "launches": sum(v["calls"] for v in convs.values()), "ms_per_step": round(tot_ms, 3),
                                    "flops": "direct-form 2*MACs of every conv / data-gradient / weight-gradient call (the layers on the "
                                             "Winograd kernels execute 4/9 of theirs: see mfma_executed)",
                                    "timing": "HIP events around each C-ABI call (kernel + its epilogue / reduction launches)"},
                    "mfma_executed": {"achieved": round(ex_gf / ex_ms, 2) if ex_ms > 0 else 0.0,
                                      "frac": round(ex_gf / ex_ms / PEAK_MFMA_F32, 4) if ex_ms > 0 else 0.0,
                                      "gflop_per_step": round(ex_gf, 1), "ms_per_step": round(ex_ms, 3),
                                      "what": "FLOPs the matrix cores execute in one step / time of the MFMA kernels themselves "
                                              "(HIP events around each main kernel; epilogue and reduction launches not included)"},
                    "by_kernel": {k: _k(k, v) for k, v in sorted(dev_k.items(), key=lambda kv: -kv[1]["ms"])[:10]},
                    "by_call_group": eager}

    if rank == 0:
        imgs = B * world * args.steps
        line = {
            "metric": "train images/sec (%dx%d, 5-frame sample, 6-scale CC step)" % (W, H),
            "value": round(imgs / dt, 3), "unit": "images/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(1e3 * dt / args.steps, 3), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": ("full CC: DispResNet6+PoseNetB6+MaskNet6+Back2Future, all losses"
                                    if args.config == "c3" else "DispResNet6+PoseNetB6, photometric+smoothness"),
                       "per_gpu_batch": B, "global_batch": B * world, "height": H, "width": W, "scales": 6,
                       "frames": 5, "parallelism": "dp%d" % world, "hipgraph": not args.no_graph,
                       "trained_nets": "disp+pose (mask, flow frozen: README --fix-masknet --fix-flownet)" if args.freeze else "all",
                       "loss": round(loss_val, 6), "rccl_ranks": dist.get_world_size() if use_dist else 1,
                       "rank_losses": rank_losses,
                       "hip_runtime": {"AMD_DIRECT_DISPATCH": os.environ.get("AMD_DIRECT_DISPATCH", "default (1)")},
                       "dead_occlusion_decoders_elided": bool(args.elide_occ), "ab_switches": ab_switches or None,
                       "net_streams": (len(tr.net_streams) if tr.net_streams else 0), "pipeline": tr.pipeline,
                       "grad_chunks": bool(getattr(tr, "grad_chunks", False)), "deterministic": bool(cc_config.deterministic)},
            "step_ms": step_ms, "comm": comm,
            "roofline": roof, "kernels": kernels,
        }
        if want_cpu:
            base, cpu_losses, cpu_first = cpu_baseline_bounded(batch_cpu, init_sd, args)
            line["cpu_baseline"] = base
            # bench-time parity gate: the engine's first steps against the oracle's on identical weights and data
            # step 0 runs both sides on IDENTICAL weights: that is the parity gate (north_star: losses within 1e-4 relative).
            # Step 1 follows one Adam update, whose first step moves every parameter by +-lr according to the SIGN of its gradient:
            # gradients of ~0 (1e-12) take either sign depending on the summation order, so the two sides' weights differ by 2*lr
            # in those elements and the losses drift apart by a few 1e-5 whatever the kernels do (tests/test_step_emu.py counts
            # those elements).  It is reported with its own, looser bound.
            par = {"tolerance": 1e-4, "tolerance_after_update": 1e-3, "steps_compared": min(len(first_losses), len(cpu_losses))}
            worst, worst_upd = 0.0, 0.0
            for i, (g_, c_) in enumerate(zip(first_losses, cpu_losses)):
                rels = {k: abs(g_[k] - c_[k]) / max(abs(c_[k]), 1e-12) for k in c_ if k in g_}
                par["step%d" % i] = {k: float("%.3e" % v) for k, v in sorted(rels.items())}
                if i == 0:
                    worst = max([worst] + list(rels.values()))
                else:
                    worst_upd = max([worst_upd] + list(rels.values()))
            par["loss_rel"] = float("%.3e" % worst) if par["steps_compared"] else None
            par["loss_rel_after_update"] = float("%.3e" % worst_upd) if par["steps_compared"] > 1 else None
            par["ok"] = bool(worst <= 1e-4 and worst_upd <= 1e-3) if par["steps_compared"] else None
            # ... so that the looser bound after the update is not the only check of the backward pass and the optimizer: the first
            # step's gradient norm per network (1e-4) and the parameters after its update (tests/test_step_emu.py's bar: Adam's first
            # step moves every parameter by lr * sign(g); elements whose ~0 gradient has the other sign end up 2 lr apart)
            if cpu_first.get("grad_norm") and len(cpu_first["grad_norm"]) == len(first_gn):
                gr = [abs(a_ - b_) / max(abs(b_), 1e-30) for a_, b_ in zip(first_gn, cpu_first["grad_norm"])]
                par["grad_norm_rel"] = [float("%.3e" % v) for v in gr]
                par["ok"] = bool(par["ok"] and max(gr) <= 1e-4)
            if "params" in cpu_first and cpu_first["params"].numel() == first_params.numel():
                gc_, ge_ = cpu_first["grads"], first_grads
                l2 = float(torch.sqrt(((ge_ - gc_).double() ** 2).sum()) / torch.sqrt((gc_.double() ** 2).sum()))
                d_ = (first_params - cpu_first["params"]).abs()
                apart = d_ > 1e-6                                   # (1 % of lr)
                # Adam's first update is lr * g / (|g| + eps): the two sides may only end up apart where their gradients have opposite
                # signs or are ~eps (elements whose value is the rounding noise of a cancelling sum); anywhere else it would be a defect
                same = (torch.sign(ge_) == torch.sign(gc_)) & (gc_.abs() > 1e-6) & (ge_.abs() > 1e-6)
                bad = int((apart & same).sum())
                par["gradient_l2_rel"] = float("%.3e" % l2)
                # where that difference sits: per network (their parameter ranges follow each other in the bucket) and how much of its
                # square the 1000 largest of the ~75 M elements carry (isolated elements: activation-derivative / bilinear-tap decisions
                # that fall the other way within rounding, tests/parity.py _flip_pinned; a kernel defect would spread)
                sizes_ = [sum(p_.numel() for p_ in n_.parameters() if p_.requires_grad) for n_ in nets if n_ is not None]
                if sum(sizes_) == ge_.numel():
                    o_, by_net = 0, []
                    for n_el in sizes_:
                        if n_el:
                            a_, b_ = ge_[o_:o_ + n_el].double(), gc_[o_:o_ + n_el].double()
                            by_net.append(float("%.3e" % float(torch.sqrt(((a_ - b_) ** 2).sum()) / torch.sqrt((b_ ** 2).sum()))))
                        o_ += n_el
                    par["gradient_l2_rel_by_net"] = by_net
                sq_ = (ge_ - gc_).double() ** 2
                par["gradient_l2_top1000_share"] = float("%.3f" % float(torch.topk(sq_, min(1000, sq_.numel())).values.sum() / sq_.sum()))
                par["update"] = {"lr": cfg.lr, "frac_apart": float("%.3e" % float(apart.float().mean())),
                                 "max_abs": float("%.4e" % float(d_.max())), "apart_with_agreeing_gradients": bad,
                                 "bar": "no element apart (> 0.01 lr) where the two gradients agree in sign and exceed 1e-6; max_abs <= 2.001 lr"}
                # bar of the whole-vector figure: 1e-3 (the per-network norms above are held to 1e-4).  Measured 5.4e-4 at B = 4,
                # 256 x 832, of which DispResNet6 7.4e-4 -- pinned in round 5 (parity.gradient_pin below, profiles/r05_grad_pin.txt): it
                # arises inside DispResNet6's backward given the REFERENCE's output gradients, does not move with the convolution
                # algorithm, and is the condition of that gradient: the reference's own fp32 evaluation is 3.8e-4 from the float64
                # gradient and moves by 2e-3 under 1e-7 input noise.  The per-network gate of the pin is the real bar.
                par["gradient_l2_bar"] = 1e-3
                par["ok"] = bool(par["ok"] and l2 <= 1e-3 and bad == 0 and float(d_.max()) <= 2.001 * cfg.lr)
            # where the whole-vector figure comes from: the reference's own d loss / d (network outputs) driven
            # through the engine's four network backward passes (i), and the engine's loss-path gradients against the reference's (ii)
            if cpu_first.get("out_grads") is not None and "grads" in cpu_first and world == 1:
                try:
                    from tools import grad_pin
                    par["gradient_pin"] = grad_pin.run(init_sd, batch_cpu, cpu_first["out_grads"], cpu_first["grads"], dev, args.config,
                                                       truth64=cpu_first.get("grads64"), cond=cpu_first.get("cond"))
                    rows_ = par["gradient_pin"]["by_net_given_reference_output_gradients"]
                    par["gradient_l2_given_ref_output_grads"] = [r_["l2_rel"] for r_ in rows_]
                    # Gate (round 6, fixed numbers): every network's parameter gradient against the EXACT (float64) gradient of the same
                    # weights and output gradients.  PoseNetB6 / MaskNet6 / Back2Future: <= 1e-4.  DispResNet6 (ReLU + BatchNorm over
                    # 16 - 208 values): its figure is made of single ReLU decisions at pre-activations within rounding of zero
                    # (profiles/r06_grad_pin.txt: two of 425 984 elements, |z| < 3e-6 against activations of 6; one of them carries 98.8 %
                    # of the squared error of its tensor), so it is gated where that can be separated: at the block boundaries with no
                    # flipped decision at or above them the engine's d loss / d (pre-activation) is held to 2.5 x the reference's own
                    # distance to float64, every flipped decision must sit at |pre-activation| <= 1e-5 of the layer's largest
                    # activation, at most 8 of them, and the whole-network figure to 2e-3.
                    if all("engine_vs_fp64" in r_ for r_ in rows_):
                        ok_small = all(r_["engine_vs_fp64"] <= 1e-4 for r_ in rows_[1:])
                        bd = grad_pin.boundaries(init_sd, batch_cpu, cpu_first["out_grads"], dev)
                        par["gradient_pin"]["dispresnet6_boundaries"] = bd["boundaries"]
                        flips = [f_ for b_ in bd["boundaries"] for f_ in b_["flips"]]
                        nflip = sum(b_["relu_flips_engine"] for b_ in bd["boundaries"])
                        clean, seen_flip = [], False
                        for b_ in reversed(bd["boundaries"]):           # deepest boundary first = the order of the backward pass
                            seen_flip = seen_flip or b_["relu_flips_engine"] > 0
                            if not seen_flip:
                                clean.append(b_)
                        ok_clean = bool(clean) and all(b_["engine_vs_fp64"] <= 2.5 * b_["reference_vs_fp64"] for b_ in clean)
                        ok_flips = nflip <= 8 and all(abs(f_["preactivation_fp64"]) <= 1e-5 * f_["max_abs_Y_fp64"] for f_ in flips
                                                      if f_.get("preactivation_fp64") is not None)
                        par["gradient_pin"]["gate"] = {
                            "pose_mask_flow_engine_vs_fp64_le_1e-4": bool(ok_small),
                            "disp_flip_free_boundaries_le_2.5x_reference": bool(ok_clean), "flip_free_boundaries": [b_["boundary"] for b_ in clean],
                            "disp_relu_flips": nflip, "disp_flips_within_rounding_of_zero": bool(ok_flips),
                            "disp_engine_vs_fp64_le_2e-3": bool(rows_[0]["engine_vs_fp64"] <= 2e-3)}
                        par["gradient_pin"]["ok"] = bool(ok_small and ok_clean and ok_flips and rows_[0]["engine_vs_fp64"] <= 2e-3)
                        par["ok"] = bool(par["ok"] and par["gradient_pin"]["ok"])
                except Exception as e:                          # noqa: BLE001 -- a diagnosis must not cost the bench line
                    par["gradient_pin"] = {"error": repr(e)}
            line["parity"] = par
        print(json.dumps(line), flush=True)
    if use_dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
