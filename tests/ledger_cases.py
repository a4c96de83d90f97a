"""The step ledger (cc_ledger_append / cc_ledger_reset_agg, cc_amd/ledger.py) and the per-parameter statistics of the flat buckets
(cc_param_stats_chunks / cc_param_stats_finish, FlatAdam.param_stats): the cases shared by tests/test_ledger.py (x86 emulation
build, CPU tensors) and tests/test_ledger_gpu.py (the product library)."""
import csv
import io

import numpy as np
import torch

from cc_amd import ledger as L, trainer as T
from grad_guard_cases import INF, backward, four_nets
from optim_hyper_cases import _sync

NAN = float("nan")
CHUNK = T.FlatAdam.PARAM_STATS_CHUNK
NAMES = L.LOSS_NAMES


# ------------------------------------------------------------------------------------------------------------------ ledger
class Sources:
    """fp32 scalars at scattered addresses of one allocation, rewritten in place before every append (what a replay of a captured
    step does to its loss tensors); `absent`: loss names that have no source"""
    SPOTS = {"step": 5, "loss": 1031, "loss_1": 77, "loss_2": 2050, "loss_3": 3, "loss_4": 4001, "loss_5": 911,
             "flag0": 64, "flag1": 1500, "flag2": 3333}

    def __init__(self, dev, absent=(), guard=False, seed=0):
        self.dev, self.absent = dev, set(absent)
        self.pool = torch.zeros(4096, dtype=torch.float32).to(dev)
        self.t = {k: self.pool[i:i + 1] for k, i in self.SPOTS.items()}
        gen = torch.Generator().manual_seed(100 + seed)
        self.hyper = torch.rand(4, 8, generator=gen).to(dev)
        self.guard = torch.rand(4, 8, generator=gen).to(dev) if guard else None
        self.gen = torch.Generator().manual_seed(seed)
        self.k = 0
        self.log = []               # per append: (n, [the six fp32 values as written into the row, absent ones 0], flag)

    def values(self):
        """six distinct fp32 values over many magnitudes (a subnormal and a negative one among them)"""
        v = (torch.randn(6, generator=self.gen) * torch.tensor([1.0, 1e-3, 1e4, 1e-20, 3.0, 1e-41])).to(torch.float32)
        return v.numpy().copy()

    def append(self, led, n, values=None, flags=(0.0, 0.0, 0.0)):
        self.k += 1
        v = self.values() if values is None else np.asarray(values, dtype=np.float32)
        self.t["step"].fill_(float(self.k))
        for name, x in zip(NAMES, v):
            self.t[name].copy_(torch.from_numpy(np.array([x], dtype=np.float32)))
        for i, f in enumerate(flags):
            self.t["flag%d" % i].fill_(f)
        losses = {name: (0 if name in self.absent else self.t[name]) for name in NAMES}
        if "loss_5" in self.absent:
            del losses["loss_5"]        # (a missing key and a non-tensor value are both "absent")
        led.append(losses, n, step=self.t["step"], nan_flags=[self.t["flag%d" % i] for i in range(3)], hyper=self.hyper, guard=self.guard)
        row = np.array([np.float32(0) if name in self.absent else x for name, x in zip(NAMES, v)], dtype=np.float32)
        self.log.append((n, row, 1.0 if any(f != 0 for f in flags) else 0.0))


def numpy_agg(log):
    """AverageMeter.update(value, n) in fp64, in step order: the same addends in the same order as the kernel's -> [7, 4]"""
    agg = np.zeros((7, 4), dtype=np.float64)
    agg[:, 2], agg[:, 3] = np.inf, -np.inf
    for n, row, flag in log:
        for c, x in enumerate(list(row) + [np.float32(flag)]):
            v = np.float64(x)
            agg[c, 0] = agg[c, 0] + np.float64(n) * v
            agg[c, 1] = agg[c, 1] + np.float64(n)
            if v < agg[c, 2]:
                agg[c, 2] = v
            if v > agg[c, 3]:
                agg[c, 3] = v
    return agg


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _same_f64(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.int64), np.ascontiguousarray(b, dtype=np.float64).view(np.int64))


def check_rows_and_aggregates(dev, guard):
    src = Sources(dev, absent=("loss_2", "loss_5"), guard=guard)
    led = L.Ledger(dev, capacity=8)
    for k in range(11):
        src.append(led, 4 if k % 2 == 0 else 3)
    d = led.drain()
    assert d.dropped == 3 and d.first_iter == 3 and tuple(d.rows.shape) == (8, 32) and d.rows.dtype == torch.float32
    rows = d.rows.numpy()
    want = np.stack([r for _, r, _ in src.log[3:]])
    assert np.array_equal(_bits(rows[:, 1:7]), _bits(want)), "a loss slot is not a bit copy of its source"
    assert np.all(rows[:, 3] == 0) and np.all(rows[:, 6] == 0) and led.absent == {"loss_2", "loss_5"}
    assert rows[:, 0].tolist() == [float(k) for k in range(4, 12)] and np.all(rows[:, 7] == 0)
    assert np.array_equal(rows[:, 8:12], np.tile(src.hyper[:, 0].cpu().numpy(), (8, 1)))
    if guard:
        g = src.guard.cpu().numpy()
        for c in range(3):
            assert np.array_equal(rows[:, 12 + 4 * c:16 + 4 * c], np.tile(g[:, c], (8, 1))), c
    else:
        assert np.all(np.isnan(rows[:, 12:24]))
    assert np.all(rows[:, 24:] == 0)
    assert L.COLUMNS[:8] == ("step", "loss", "loss_1", "loss_2", "loss_3", "loss_4", "loss_5", "nan") and len(L.COLUMNS) == 32
    assert L.COLUMNS[8] == "lr_disp" and L.COLUMNS[13] == "norm_pose" and L.COLUMNS[18] == "coef_mask" and L.COLUMNS[23] == "finite_flow"
    again = led.drain()
    assert again.rows.shape[0] == 0 and again.dropped == 0 and again.first_iter == 11
    # the aggregates saw all eleven rows: exact, the addends and their order are the kernel's
    want_agg = numpy_agg(src.log)
    got = led.agg.cpu().numpy()
    assert _same_f64(got, want_agg), (got, want_agg)
    avg = led.average()
    assert list(avg) == list(NAMES) + ["nan"]
    for c, name in enumerate(NAMES):
        assert avg[name] == {"avg": want_agg[c, 0] / want_agg[c, 1], "min": want_agg[c, 2], "max": want_agg[c, 3], "weight": 39.0}
    # 5 more: only those come back
    for k in range(5):
        src.append(led, 4)
    d = led.drain()
    assert d.first_iter == 11 and d.dropped == 0 and d.rows[:, 0].tolist() == [12.0, 13.0, 14.0, 15.0, 16.0]


def check_resets(dev):
    src = Sources(dev, seed=1)
    led = L.Ledger(dev, capacity=8)
    for k in range(2):
        src.append(led, 4)
    led.reset_average()                 # (no sync on either side of it: ordered on the stream)
    for k in range(3):
        src.append(led, 3)
    assert _same_f64(led.agg.cpu().numpy(), numpy_agg(src.log[2:]))
    # a resumed run: head and the aggregates continue, the ring does not travel
    sd = led.state_dict()
    assert sd["head"] == 5 and tuple(sd["agg"].shape) == (7, 4) and sd["agg"].dtype == torch.float64
    led2 = L.Ledger(dev, capacity=8)
    led2.load_state_dict(sd)
    src.append(led2, 4)
    d = led2.drain()
    assert d.first_iter == 5 and d.dropped == 0 and d.rows.shape[0] == 1 and float(d.rows[0, 0]) == 6.0
    assert _same_f64(led2.agg.cpu().numpy(), numpy_agg(src.log[2:]))
    assert led2.average()["loss"]["weight"] == 13.0
    led2.reset_average()
    a = led2.average()["loss_3"]
    assert a["weight"] == 0.0 and a["avg"] == 0.0 and a["min"] == INF and a["max"] == -INF
    for bad in (0, 12, -8):
        try:
            L.Ledger(dev, capacity=bad)
        except ValueError:
            continue
        raise AssertionError("capacity %r accepted" % (bad,))


def check_nonfinite(dev):
    src = Sources(dev, seed=2)
    led = L.Ledger(dev, capacity=8)
    src.append(led, 4)
    v = src.values()
    v[3] = np.float32(NAN)                              # loss_3
    src.append(led, 3, values=v, flags=(0.0, 2.0, 0.0))
    src.append(led, 4, flags=(0.0, 0.0, 0.0))
    rows = led.drain().rows.numpy()
    assert np.isnan(rows[1, 4]) and not np.isnan(np.delete(rows, 4, axis=1)[:, :11]).any()
    assert rows[:, 7].tolist() == [0.0, 1.0, 0.0]
    got, want = led.agg.cpu().numpy(), numpy_agg(src.log)
    assert np.isnan(got[3, 0]) and got[3, 1] == 11.0
    assert _same_f64(np.delete(got, 3, axis=0), np.delete(want, 3, axis=0))
    assert got[3, 2] == want[3, 2] and got[3, 3] == want[3, 3]        # min / max of the finite values
    assert got[6].tolist() == [3.0, 11.0, 0.0, 1.0]                   # the NaN indicator: 3 of 11 samples
    assert np.isnan(led.average()["loss_3"]["avg"])


def check_log_file(dev, tmp_path):
    for case, absent in (("full", ()), ("w2_zero", ("loss_2",))):
        src = Sources(dev, absent=absent, seed=3)
        led = L.Ledger(dev, capacity=8)
        for k in range(4):
            src.append(led, 4)
        path = tmp_path / ("progress_log_full_%s.csv" % case)
        d = led.drain()
        led.write_log_full(path, d.rows[:2])
        led.write_log_full(path, d.rows[2:])                # (appends)
        buf = io.StringIO(newline="")
        w = csv.writer(buf, delimiter="\t")
        for _, r, _ in src.log:
            w.writerow([float(r[0]), float(r[1]), float(r[2]) if not absent else 0, float(r[3]), float(r[4])])
        got = open(path, "rb").read()
        assert got == buf.getvalue().encode(), (case, got, buf.getvalue())
        if absent:
            assert all(line.split(b"\t")[2] == b"0" for line in got.split(b"\r\n")[:-1])


def check_ledger_follows_flat_adam(dev):
    """The trainer's wiring on the tiny networks of the guard cases: the row reads FlatAdam's counter, table and guard rows behind
    the step -- step slot 1, 2, 3; the lr slots follow a set_hyper between steps 2 and 3; the norm slots are grad_stats()'s."""
    nets = four_nets(dev)
    opt = T.FlatAdam(nets, T.StepConfig(max_grad_norm=INF))
    led = L.Ledger(dev, capacity=4)
    loss = torch.zeros(1, dtype=torch.float32).to(dev)
    stats = []
    for s in range(3):
        if s == 2:
            opt.set_hyper("pose", lr=3e-3)
        backward(opt, nets, dev, s + 1)
        opt.step()
        loss.fill_(0.5 * (s + 1))
        led.append({"loss": loss}, 2, step=opt.step_dev, hyper=opt.hyper_dev, guard=opt.guard_dev)
        stats.append(opt.grad_stats(sync=True))
    rows = led.drain().rows
    assert rows[:, 0].tolist() == [1.0, 2.0, 3.0] and rows[:, 1].tolist() == [0.5, 1.0, 1.5]
    lr = np.float32(1e-4)
    assert rows[:, 8:12].tolist() == [[lr] * 4, [lr] * 4, [lr, np.float32(3e-3), lr, lr]]
    for s in range(3):
        assert rows[s, 12:16].tolist() == [stats[s][k]["norm"] for k in T.NET_NAMES]
        assert rows[s, 16:20].tolist() == [1.0] * 4 and rows[s, 20:24].tolist() == [1.0] * 4
    assert led.absent == set(NAMES[1:])


# ---------------------------------------------------------------------------------------------------- parameter statistics
class Bag(torch.nn.Module):
    def __init__(self, sizes, seed):
        super().__init__()
        gen = torch.Generator().manual_seed(seed)
        self.w = torch.nn.ParameterList([torch.nn.Parameter(0.1 * torch.randn(k, generator=gen)) for k in sizes])


# the first network: offsets 0, 1, 4, 9 (a start 1 float, then 0, then 1 float behind a 16-byte boundary), then C + 1 elements
# from offset 13 and 4096 from an odd offset; it ends 50 floats in front of the next 256-byte boundary (padding).  The second: C,
# then 2C + 5 (three chunks, the last one 5 elements) from an aligned start, then single elements
SIZES = [[1, 3, 5, 4, CHUNK + 1, 4096], [CHUNK, 2 * CHUNK + 5, 1, 1]]


def bucket(dev):
    nets = [Bag(s, 7 + i).to(dev) for i, s in enumerate(SIZES)]
    opt = T.FlatAdam(nets, T.StepConfig())
    gen = torch.Generator().manual_seed(5)
    opt.flat_g.copy_((0.05 * torch.randn(opt.flat_g.numel(), generator=gen)).to(dev))
    lo, hi = opt.net_ranges[0][1], opt.net_ranges[1][0]
    assert hi - lo >= 2 and sum(1 for o in opt.offsets if o % 4) >= 4
    return nets, opt


def _prefill_nan(opt):
    t = opt._param_stats_tables()
    t["partials"].fill_(NAN)
    t["stats"].fill_(NAN)


def _reference(opt, scale):
    out = []
    for p, off in zip(opt.params, opt.offsets):
        g, w = opt.flat_g[off:off + p.numel()].double().cpu(), opt.flat_p[off:off + p.numel()].double().cpu()
        fin = torch.isfinite(g)
        out.append({"grad_norm": scale * float(g.pow(2).sum().sqrt()), "weight_norm": float(w.pow(2).sum().sqrt()),
                    "grad_maxabs": float(g[~torch.isnan(g)].abs().max()) if bool((~torch.isnan(g)).any()) else 0.0,
                    "nonfinite": float((~fin).sum()), "n": p.numel()})
    return out


def check_param_stats(dev):
    nets, opt = bucket(dev)
    names = ["disp.w.%d" % i for i in range(len(SIZES[0]))] + ["pose.w.%d" % i for i in range(len(SIZES[1]))]
    assert opt.param_names == names
    _prefill_nan(opt)
    views = opt.param_stats(grad_scale=0.5)
    v = views["pose.w.1"]["grad_norm"]
    assert torch.is_tensor(v) and v.dim() == 0 and v.dtype == torch.float64 and v.device.type == torch.device(dev).type
    first = opt._pstats["stats"].clone()
    _prefill_nan(opt)
    got = opt.param_stats(grad_scale=0.5, sync=True)
    _sync(dev)
    assert torch.equal(first.view(torch.int64), opt._pstats["stats"].view(torch.int64)), "two calls on the same buckets differ"
    assert list(got) == names
    nchunks = sum(-(-k // CHUNK) for s in SIZES for k in s)
    assert tuple(opt._pstats["chunks"].shape) == (nchunks, 2) and int(opt._pstats["chunks"][:, 1].max()) == CHUNK
    for name, ref in zip(names, _reference(opt, 0.5)):
        g = got[name]
        tol = ref["n"] * 2.0 ** -52             # fp64 summation of n non-negative terms, any order
        for k in ("grad_norm", "weight_norm"):
            rel = abs(g[k] - ref[k]) / ref[k]
            assert rel <= tol, (name, k, g[k], ref[k], rel, tol)
        assert g["grad_maxabs"] == ref["grad_maxabs"] and g["nonfinite"] == 0.0, (name, g, ref)
    assert opt.first_nonfinite() is None and int(opt.first_nonfinite(sync=False)) == -1
    # grad_scale None: 1 / world size
    assert opt.param_stats(sync=True)["disp.w.4"]["grad_norm"] == 2.0 * got["disp.w.4"]["grad_norm"]


def check_param_stats_nonfinite(dev):
    nets, opt = bucket(dev)
    off = opt.offsets
    opt.flat_g[off[5]] = NAN                            # first element of disp.w.5 ...
    opt.flat_g[off[5] - 1] = INF                        # ... and the last one of disp.w.4 (its chunk of ONE element)
    pad = opt.net_ranges[0][1]
    opt.flat_g[pad] = NAN                               # alignment padding between the networks: nobody's
    _prefill_nan(opt)
    got = opt.param_stats(grad_scale=1.0, sync=True)
    ref = _reference(opt, 1.0)
    for j, (name, r) in enumerate(zip(opt.param_names, ref)):
        g = got[name]
        assert g["nonfinite"] == (1.0 if j in (4, 5) else 0.0), (name, g)
        if j not in (4, 5):
            assert np.isfinite(g["grad_norm"]) and abs(g["grad_norm"] - r["grad_norm"]) <= r["n"] * 2.0 ** -52 * r["grad_norm"], (name, g, r)
        assert g["grad_maxabs"] == r["grad_maxabs"] and abs(g["weight_norm"] - r["weight_norm"]) <= r["n"] * 2.0 ** -52 * r["weight_norm"]
    assert got["disp.w.4"]["grad_norm"] == INF and got["disp.w.4"]["grad_maxabs"] == INF and np.isnan(got["disp.w.5"]["grad_norm"])
    assert opt.first_nonfinite() == "disp.w.4" and int(opt.first_nonfinite(sync=False)) == 4
    opt.flat_g[off[5] - 1] = 0.0
    assert opt.first_nonfinite() == "disp.w.5"
