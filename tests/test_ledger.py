"""The step ledger and the per-parameter statistics on CPU tensors through the x86 emulation build of the kernel sources.  The
trainer-wiring checks of tests/test_ledger_gpu.py (a full CC step on the CPU takes minutes) are replaced here by
test_ledger_reads_flat_adams_tables, which drives the same sources -- FlatAdam's counter, hyperparameter table and guard rows --
through FlatAdam.step() on the tiny networks of the guard cases."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import ledger_cases as C
from cc_amd import ledger as L, trainer as T
from hipemu.emu import emulated_engine

DEV = "cpu"


@pytest.mark.parametrize("guard", [False, True])
def test_rows_and_aggregates(guard):
    with emulated_engine():
        C.check_rows_and_aggregates(DEV, guard)


def test_resets_and_resume():
    with emulated_engine():
        C.check_resets(DEV)


def test_non_finite_values():
    with emulated_engine():
        C.check_nonfinite(DEV)


def test_log_file_is_the_references(tmp_path):
    with emulated_engine():
        C.check_log_file(DEV, tmp_path)


def test_ledger_reads_flat_adams_tables():
    with emulated_engine():
        C.check_ledger_follows_flat_adam(DEV)


def test_step_config_default_is_off():
    assert T.StepConfig().ledger is None and T.StepConfig(ledger=64).ledger == 64
    with emulated_engine():
        nets = T.build_nets(DEV, flow=False, mask=False, init=True)
        assert T.CCTrainer(nets, T.StepConfig(), use_graph=False).ledger is None
        tr = T.CCTrainer(nets, T.StepConfig(ledger=16), use_graph=False)
        assert isinstance(tr.ledger, L.Ledger) and tr.ledger.capacity == 16 and int(tr.ledger.head) == 0
        led = tr.ledger
        tr.switch_pipeline("post")
        assert tr.ledger is led
        with pytest.raises(ValueError):
            T.CCTrainer(nets, T.StepConfig(ledger=12), use_graph=False)


def test_param_stats_synthetic_bucket():
    with emulated_engine():
        C.check_param_stats(DEV)


def test_param_stats_non_finite_placement():
    with emulated_engine():
        C.check_param_stats_nonfinite(DEV)


# ---------------------------------------------------------------------------------------------------------- two gloo ranks
def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def _worker(rank, world, port, ret):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    with emulated_engine():
        src = C.Sources(DEV, seed=10 + rank, guard=True)
        src.hyper.fill_(0.25)
        src.guard.fill_(0.5)                # (lr and guard columns: the same on every rank)
        led = L.Ledger(DEV, capacity=8)
        for k in range(3):                  # (a NaN flag on rank 1 alone, in the second step: both ranks have to see it)
            src.append(led, 4, flags=(0.0, 1.0, 0.0) if (rank == 1 and k == 1) else (0.0, 0.0, 0.0))
        d = led.drain(reduce="mean")
        out = {"rows": d.rows.clone(), "first": d.first_iter, "dropped": d.dropped, "own": [r for _, r, _ in src.log]}
        for _ in range(2 if rank == 1 else 1):          # rank 1 is one row ahead
            src.append(led, 4)
        try:
            led.drain(reduce="mean")
            out["raised"] = None
        except RuntimeError as e:
            out["raised"] = str(e)
        ret[rank] = out
    dist.destroy_process_group()


def test_drain_mean_over_two_ranks():
    import numpy as np
    world, port = 2, _free_port()
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(world, port, ret), nprocs=world, join=True)
    r0, r1 = ret[0], ret[1]
    assert r0["first"] == r1["first"] == 0 and r0["dropped"] == r1["dropped"] == 0
    assert torch.equal(r0["rows"].view(torch.int32), r1["rows"].view(torch.int32))
    want = (np.stack(r0["own"]) + np.stack(r1["own"])) / np.float32(2)
    assert want.dtype == np.float32 and not np.array_equal(np.stack(r0["own"]), np.stack(r1["own"]))
    assert np.array_equal(r0["rows"][:, 1:7].numpy(), want)
    assert r0["rows"][:, 7].tolist() == [0.0, 1.0, 0.0]
    assert r0["rows"][:, 0].tolist() == [1.0, 2.0, 3.0] and r0["rows"][:, 8:12].eq(0.25).all() and r0["rows"][:, 12:24].eq(0.5).all()
    for r in (r0, r1):
        assert r["raised"] is not None and "same iteration" in r["raised"], r["raised"]
