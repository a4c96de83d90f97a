"""FlowNetC6 in the trainer's step on the x86 emulation build (tests/flownetc_cases.py): the plane-GEMM cost-volume kernels against
float64 and the gather kernels, the torch restatement against the reference's fixtures, forward_pair, the eager step and the
forward-only validation pass against the oracle, and Back2Future's step untouched by the new switch."""
import pytest

import flownetc_cases as FC
from hipemu.emu import emulated_engine


@pytest.mark.parametrize("case", FC.KERNEL_CASES, ids=["x".join(map(str, c)) for c in FC.KERNEL_CASES])
def test_plane_kernels_against_float64(case):
    with emulated_engine():
        FC.check_kernels("cpu", case)


def test_refused_shape_falls_through_to_the_gather_kernels():
    with emulated_engine():
        FC.check_fall_through("cpu")


def test_restatement_matches_the_reference_fixtures(golden_dir):
    FC.check_restatement_against_golden(golden_dir)


@pytest.mark.slow          # (the 2 x 64 x 128 networks on the emulation build)
def test_forward_pair_equals_two_calls():
    with emulated_engine():
        FC.check_forward_pair("cpu")


@pytest.mark.slow          # (the 2 x 64 x 128 networks on the emulation build)
def test_step_against_oracle():
    with emulated_engine():
        FC.check_step_against_oracle("cpu")


def test_legacy_pipelines_refuse_a_two_frame_flow_network():
    with emulated_engine():
        FC.check_legacy_forms_refused("cpu")


@pytest.mark.slow          # (the 2 x 64 x 128 networks on the emulation build)
def test_validation_pass_against_oracle(tmp_path):
    with emulated_engine():
        FC.check_validation_pass("cpu", tmp_path)


def test_back2future_step_unmoved_by_the_switch():
    with emulated_engine():
        FC.check_back2future_step_unmoved("cpu")
