"""Data preparation (cc_amd/datasets/prepare.py, python -m cc_amd.prepare) on the x86 emulation build of the kernels, device "cpu":
the uint8 resize against Pillow itself, KITTI raw (both frame-selection rules, with ground truth) and Cityscapes end to end against
what the unmodified reference script wrote for the same trees (tests/golden/prepare_*.npz, tools/make_prepare_golden.py), the
stores written beside the folders, and the command line.  tests/prepare_cases.py holds the cases; the same ones run on the GPU in
tests/test_prepare_gpu.py."""
import pytest

import prepare_cases as C
from hipemu.emu import emulated_engine


@pytest.fixture(scope="module")
def emu():
    with emulated_engine():
        yield


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    return tmp_path_factory.mktemp("prepare_src")


def test_resize_u8_is_pillow_bilinear_emulated(emu):
    C.check_resize("cpu")


def test_resize_u8_argument_errors_emulated(emu):
    C.check_resize_errors("cpu")


@pytest.mark.parametrize("run", ["kitti_speed", "kitti_static"])
def test_kitti_matches_reference_emulated(emu, trees, tmp_path, golden_dir, run):
    C.check_kitti("cpu", trees, tmp_path, golden_dir, run)


def test_cityscapes_matches_reference_emulated(emu, trees, tmp_path, golden_dir):
    C.check_cityscapes("cpu", trees, tmp_path, golden_dir)


def test_stores_equal_stores_built_off_the_folders_emulated(emu, trees, tmp_path, golden_dir):
    C.check_stores("cpu", trees, tmp_path, golden_dir)


def test_parser_has_the_reference_options():
    C.check_parser()


def test_cli_refuses_kitti_without_test_scenes(capsys):
    C.check_cli_refuses_kitti_without_test_scenes(capsys)


def test_cli_end_to_end_emulated(emu, trees, tmp_path, golden_dir, capsys):
    C.check_cli_run("cpu", trees, tmp_path, golden_dir, capsys)


def test_greyscale_png_is_refused_by_name_emulated(emu, tmp_path):
    C.check_grey_png("cpu", tmp_path)
