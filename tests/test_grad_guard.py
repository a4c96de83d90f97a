"""The gradient guard of the Adam step (per-network gradient norm, clipping, NaN / Inf skip) on CPU tensors through the x86 emulation
build of the kernel sources; clip_grad_norm_ + torch.optim.Adam are the reference."""
import pytest
import torch

import grad_guard_cases as C
from cc_amd import config, trainer as T
from hipemu.emu import emulated_engine

DEV = "cpu"


@pytest.mark.parametrize("n", C.NORM_SIZES)
def test_norm_is_the_fp64_norm_and_deterministic(n):
    with emulated_engine():
        C.check_norm(n, DEV)


def test_clip_and_adam_match_clip_grad_norm_and_torch_adam():
    """rows clipped to half their norm / far below their bound / with max_grad_norm = inf, three steps: within 1e-6 absolute of
    clip_grad_norm_ + torch.optim.Adam per slice (test_rows_and_bounds' bound for these magnitudes; torch's fp32 run is within it
    of its fp64 run); the rows with coef == 1 are cc_adam_step_segment_hyper's bits"""
    with emulated_engine():
        C.check_clip_against_torch(DEV)


def test_non_finite_rows_are_left_alone():
    """clean / NaN in row 1 + Inf in row 2 (each the row's last element) / clean"""
    with emulated_engine():
        C.check_skip(DEV)


def test_flat_adam_guard_off_is_todays_optimizer():
    with emulated_engine():
        C.check_guard_off_surface(DEV)


def test_flat_adam_guard_on_surface():
    with emulated_engine():
        C.check_guard_on_surface(DEV)


def test_step_config_default_is_off():
    assert T.StepConfig().max_grad_norm is None and T.StepConfig(max_grad_norm=5.0).max_grad_norm == 5.0
    with pytest.raises(ValueError):
        with emulated_engine():
            T.FlatAdam(C.four_nets(DEV), T.StepConfig(max_grad_norm=0.0))


def test_grad_chunks_with_the_guard_raise(monkeypatch):
    """construction only: a chunk's update would start before the network's norm exists"""
    monkeypatch.setattr(config, "grad_chunks", True)
    with emulated_engine():
        nets = T.build_nets(DEV, flow=False, mask=False, init=True)
        with pytest.raises(ValueError, match="gradient chunks"):
            T.CCTrainer(nets, T.StepConfig(max_grad_norm=1.0), use_graph=False)
        monkeypatch.setattr(config, "grad_chunks", False)
        tr = T.CCTrainer(nets, T.StepConfig(max_grad_norm=1.0), use_graph=False)
        with pytest.raises(ValueError, match="gradient chunks"):
            tr.set_grad_chunks(True)
        assert not tr.grad_chunks and tr._chunk_lo == {}
        tr.set_grad_chunks(False)
        with pytest.raises(ValueError):
            T.CCTrainer(T.build_nets(DEV, flow=False, mask=False, init=True), T.StepConfig(), use_graph=False).grad_stats()
