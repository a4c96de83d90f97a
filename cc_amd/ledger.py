"""Step ledger: the per-step scalars of a training run, recorded on the device (cc_amd/csrc/ledger.hip).

train.py:563,574-576 reads the losses back with ``.item()`` in every iteration.  A captured step overwrites its loss tensors with
every replay, so following the reference's log means one host sync between two replays.  The ledger's append is the last launch of
the step (a node of the captured graph): it writes one row of 32 floats into a ring in device memory and folds the loss columns
into fp64 aggregates (``AverageMeter.update(loss, batch_size)``).  The host reads the ring when it wants to -- ``drain()`` every
``print_freq`` steps, ``average()`` once per epoch -- and nothing is lost in between as long as it drains at least once per
`capacity` steps (what was overwritten is reported as ``dropped``, never silently).
"""
import collections
import csv
import ctypes

import torch
import torch.distributed as dist

from ._lib import engine, header_constant, STREAM

SLOTS = header_constant("CC_LEDGER_SLOTS")
NETS = ("disp", "pose", "mask", "flow")
LOSS_NAMES = ("loss", "loss_1", "loss_2", "loss_3", "loss_4", "loss_5")
# the row layout (slot -> name); the slots behind the last name are zero
COLUMNS = ("step",) + LOSS_NAMES + ("nan",) + tuple("lr_" + n for n in NETS) + tuple("norm_" + n for n in NETS) + \
    tuple("coef_" + n for n in NETS) + tuple("finite_" + n for n in NETS)
COLUMNS = COLUMNS + (None,) * (SLOTS - len(COLUMNS))
# the aggregated columns: slots 1..7 -- the six losses (loss is the total) and the NaN indicator, whose weighted mean is the share of
# samples whose step raised a NaN flag
AGG_NAMES = LOSS_NAMES + ("nan",)
_AGG_ROWS = header_constant("CC_LEDGER_AGG_ROWS")
_SRC_FLAGS = header_constant("CC_LEDGER_SRC_FLAGS")
_MAX_SOURCES = header_constant("CC_LEDGER_MAX_SOURCES")
assert len(AGG_NAMES) == _AGG_ROWS and len(COLUMNS) == SLOTS
_HEAD_BYTES, _AGG_BYTES = 16, _AGG_ROWS * 4 * 8           # layout of the state buffer: head (+ 8 bytes of padding) | agg | ring

Drained = collections.namedtuple("Drained", "rows first_iter dropped")


class Ledger:
    """A ring of `capacity` rows of 32 floats (COLUMNS), a count of the rows ever appended (`head`: the reference's n_iter) and the
    running fp64 aggregates {weighted sum, weight, min, max} of the loss columns -- all in ONE device buffer (`state`) that is
    allocated here, never during a capture.  Usable without a trainer."""

    def __init__(self, device, capacity=4096):
        capacity = int(capacity)
        if capacity <= 0 or capacity & (capacity - 1):
            raise ValueError("Ledger: capacity must be a power of two, got %r" % (capacity,))
        self.device, self.capacity = torch.device(device), capacity
        self.state = torch.zeros(_HEAD_BYTES + _AGG_BYTES + capacity * SLOTS * 4, dtype=torch.uint8, device=self.device)
        self.head = self.state[:8].view(torch.int64)
        self.agg = self.state[_HEAD_BYTES:_HEAD_BYTES + _AGG_BYTES].view(torch.float64).view(_AGG_ROWS, 4)
        self.ring = self.state[_HEAD_BYTES + _AGG_BYTES:].view(torch.float32).view(capacity, SLOTS)
        self.agg[:, 2], self.agg[:, 3] = float("inf"), -float("inf")
        self._host = torch.zeros(self.state.numel(), dtype=torch.uint8)       # what drain() copies into: page-locked on a HIP device
        if self.device.type == "cuda":
            self._host = self._host.pin_memory()
        self._drained = 0           # value of head at the previous drain
        self.absent = set()         # names of the loss terms the MOST RECENT append had no source for (written as 0)

    # ------------------------------------------------------------------------------------------------------------ device side
    def append(self, losses, n, step=None, nan_flags=(), hyper=None, guard=None):
        """One launch on the current stream (capturable): row head % capacity = the values the sources hold when the launch runs.
        losses: {'loss', 'loss_1', .. 'loss_5': 1-element fp32 tensor}; a missing name or a value that is not a tensor (train.py:495
        ``loss_2 = 0``) is written as 0 and named in `absent`.  n: the weight of the step in the averages (the batch size).
        step: FlatAdam.step_dev; nan_flags: 1-element fp32 tensors (at most 23); hyper / guard: FlatAdam.hyper_dev / guard_dev
        ([rows <= 4, 8]; guard None: the norm / coef / finite slots are NaN, "not measured")."""
        E = engine()
        flags = list(nan_flags)
        if len(flags) > _MAX_SOURCES - _SRC_FLAGS:
            raise ValueError("Ledger.append: %d NaN flags, at most %d fit into one row's sources" % (len(flags), _MAX_SOURCES - _SRC_FLAGS))
        srcs = [step] + [losses.get(k) if torch.is_tensor(losses.get(k)) else None for k in LOSS_NAMES] + [hyper, guard] + flags
        self.absent = {k for k, t in zip(LOSS_NAMES, srcs[1:7]) if t is None}
        rows = 0
        for t in (hyper, guard):
            if t is not None:
                if t.dim() != 2 or t.shape[1] != 8 or t.shape[0] > 4 or (rows and t.shape[0] != rows):
                    raise ValueError("Ledger.append: hyper / guard must be [rows <= 4, 8] tables of the same height")
                rows = t.shape[0]
        for t in srcs[:7] + flags:
            if t is not None and (t.dtype != torch.float32 or t.numel() != 1):
                raise TypeError("Ledger.append: a scalar source must be a 1-element fp32 tensor")
        arr = (ctypes.c_long * len(srcs))(*[(E._ptr(t, "cc_ledger_append", k) if t is not None else 0) for k, t in enumerate(srcs)])
        E.call("cc_ledger_append", ctypes.addressof(arr), len(srcs), rows, int(n), self.ring, self.capacity, self.head, self.agg, STREAM)

    def reset_average(self):
        """a new AverageMeter (train.py:426, once per epoch), ordered on the current stream"""
        engine().call("cc_ledger_reset_agg", self.agg, STREAM)

    # -------------------------------------------------------------------------------------------------------------- host side
    def _read(self):
        """head + aggregates + ring -> the host buffer: one stream-ordered copy, one event wait"""
        self._host.copy_(self.state, non_blocking=True)
        if self.device.type == "cuda":
            ev = torch.cuda.Event()
            ev.record()
            ev.synchronize()
        head = int(self._host[:8].view(torch.int64)[0])
        ring = self._host[_HEAD_BYTES + _AGG_BYTES:].view(torch.float32).view(self.capacity, SLOTS)
        return head, ring

    def drain(self, reduce=None):
        """-> Drained(rows, first_iter, dropped): the rows appended since the previous drain, oldest first, as a float32 tensor
        [k, 32] on the host; first_iter = the value of head at the first returned row; dropped = how many rows were overwritten
        before they could be drained (append more than `capacity` rows between two drains and the oldest are gone).
        reduce='mean' (data-parallel): the loss columns averaged over the process group -- all ranks call it at the same
        iteration; raises if first_iter or the number of rows differ between the ranks.  The NaN indicator (slot 7) becomes 1 if
        ANY rank raised a flag in that step (the photometric terms are per rank).  (The lr, norm, coef and finite columns are the
        same on every rank already: they come from the all-reduced gradient.)"""
        if reduce not in (None, "mean"):
            raise ValueError("Ledger.drain: reduce must be None or 'mean', got %r" % (reduce,))
        head, ring = self._read()
        dropped = max(0, head - self._drained - self.capacity)
        first = self._drained + dropped
        idx = torch.arange(first, head, dtype=torch.int64) & (self.capacity - 1)
        rows = ring[idx].clone()
        self._drained = head
        if reduce == "mean" and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            rows = self._mean_over_ranks(rows, first)
        return Drained(rows, first, dropped)

    def _mean_over_ranks(self, rows, first):
        world = dist.get_world_size()
        on_dev = dist.get_backend() == "nccl"           # (RCCL's process group moves device tensors only)
        mine = torch.tensor([first, rows.shape[0]], dtype=torch.int64)
        mine = mine.to(self.device) if on_dev else mine
        every = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)
        seen = [tuple(int(v) for v in t.tolist()) for t in every]
        if any(s != seen[0] for s in seen):
            raise RuntimeError("Ledger.drain(reduce='mean'): the ranks are not at the same iteration -- (first_iter, rows) per rank: %s"
                               % (seen,))
        if rows.shape[0]:
            k = len(LOSS_NAMES)
            part = rows[:, 1:2 + k].contiguous()                # the six losses and the 0 / 1 indicator: one SUM all-reduce
            part = part.to(self.device) if on_dev else part
            dist.all_reduce(part)
            part = part.cpu()
            rows[:, 1:1 + k] = part[:, :k] / world
            rows[:, 1 + k] = (part[:, k] > 0).to(torch.float32)      # (a sum of 0 / 1 values > 0: the maximum over the ranks)
        return rows

    def average(self):
        """{'loss', 'loss_1' .. 'loss_5', 'nan': {'avg', 'min', 'max', 'weight'}} since the last reset_average(): avg = the fp64
        weighted mean (AverageMeter.avg, train.py:586 returns losses.avg[0] = average()['loss']['avg']); one read-back."""
        agg = self.agg.cpu().tolist()
        return {k: {"avg": (s / w if w > 0 else 0.0), "min": lo, "max": hi, "weight": w} for k, (s, w, lo, hi) in zip(AGG_NAMES, agg)}

    def state_dict(self):
        return {"head": int(self.head.cpu()[0]), "agg": self.agg.detach().cpu().clone(), "capacity": self.capacity}

    def load_state_dict(self, sd):
        """continue a run: n_iter (head) and the running averages; the rows of the ring are not part of a checkpoint"""
        if self.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("Ledger.load_state_dict: a hipGraph capture is in progress")
        self.head.fill_(int(sd["head"]))
        self.agg.copy_(sd["agg"])
        self._drained = int(sd["head"])

    def write_log_full(self, path, rows):
        """Append the lines of train.py:574-576 (progress_log_full.csv) for `rows` (a drain()'s rows): tab-separated
        [loss, loss_1, loss_2 or 0, loss_3, loss_4] as csv.writer formats the Python floats ``.item()`` returns.  Whether loss_2
        is written as the reference's integer 0 is decided by `absent` as it is NOW (every append overwrites it), not as it was
        when the rows were recorded: a bare Ledger fed with changing sets of sources has to write its rows before the set changes
        (a trainer's set is fixed by its configuration)."""
        with open(path, "a") as f:
            w = csv.writer(f, delimiter="\t")
            for r in rows.tolist():         # (float32 -> Python float: the value .item() gives)
                w.writerow([r[1], r[2], 0 if "loss_2" in self.absent else r[3], r[4], r[5]])
