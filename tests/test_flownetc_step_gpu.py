"""FlowNetC6 in the trainer's step on the MI355X (tests/flownetc_cases.py): what tests/test_flownetc_step.py runs on the emulation
build, plus the captured step -- three replays equal three eager steps bit for bit in config.deterministic mode."""
import pytest

import flownetc_cases as FC

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("case", FC.KERNEL_CASES, ids=["x".join(map(str, c)) for c in FC.KERNEL_CASES])
def test_plane_kernels_against_float64(case):
    FC.check_kernels(DEV, case)


def test_refused_shape_falls_through_to_the_gather_kernels():
    FC.check_fall_through(DEV)


def test_forward_pair_equals_two_calls():
    FC.check_forward_pair(DEV)


def test_step_against_oracle():
    FC.check_step_against_oracle(DEV)


def test_captured_step_equals_eager_steps(monkeypatch):
    FC.check_captured_equals_eager(DEV, monkeypatch)


def test_validation_pass_against_oracle(tmp_path):
    FC.check_validation_pass(DEV, tmp_path)


def test_back2future_step_unmoved_by_the_switch():
    FC.check_back2future_step_unmoved(DEV)
