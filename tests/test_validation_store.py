"""The ragged-batch flow metrics, the validation folder, the resident validation stores and the loops over them, on the host and on
the x86 emulation build of the kernels (tests/validation_store_cases.py holds the cases; the same ones run on the GPU in
tests/test_validation_store_gpu.py).  The folder's order is compared with the fixture the unmodified reference wrote
(tests/golden/validation_folder.json, tools/make_validation_golden.py)."""
import pytest

import validation_store_cases as C
from hipemu.emu import emulated_engine


@pytest.fixture(scope="module")
def emu():
    with emulated_engine():
        yield


def test_samples_rows_equal_single_sample_calls_emulated(emu):
    C.check_rows_exact("cpu")


def test_samples_rows_against_reference_arithmetic_emulated(emu):
    C.check_rows_against_oracle("cpu", 1e-6)


def test_samples_meter_emulated(emu):
    C.check_meter("cpu")


def test_samples_argument_errors_emulated(emu):
    C.check_argument_errors("cpu")


def test_validation_set_matches_reference(tmp_path, golden_dir):
    C.check_validation_set(C.build_val_tree(tmp_path / "val"), golden_dir)


def test_depth_store_emulated(emu, tmp_path):
    C.check_depth_store("cpu", tmp_path)


def test_flow_store_emulated(emu, tmp_path):
    C.check_flow_store("cpu", tmp_path)


def test_flow_cli_parses_the_store_flags():
    from cc_amd import kitti_eval as K
    base = ["flow", "--kitti-dir", "K", "--pretrained-disp", "d", "--pretrained-pose", "p", "--pretrained-mask", "m", "--pretrained-flow", "f"]
    a = K.parser().parse_args(base)
    assert (a.batch_size, a.cache) == (1, None)
    a = K.parser().parse_args(base + ["--batch-size", "8", "--cache", "DIR"])
    assert (a.batch_size, a.cache) == (8, "DIR")
