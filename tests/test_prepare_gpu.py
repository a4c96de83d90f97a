"""Data preparation on the GPU: the cases of tests/prepare_cases.py on the real library, the resize at KITTI and Cityscapes sizes
(375 x 1242 -> 256 x 832, 1024 x 2048 -> 171 x 416 with 128 rows kept), and one training batch from the prepared train store."""
import pytest

import prepare_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    return tmp_path_factory.mktemp("prepare_src")


def test_resize_u8_is_pillow_bilinear_gpu():
    C.check_resize("cuda")


def test_resize_u8_dataset_sizes_gpu():
    C.check_resize("cuda", C.RESIZE_CASES_BIG)


def test_resize_u8_argument_errors_gpu():
    C.check_resize_errors("cuda")


@pytest.mark.parametrize("run", ["kitti_speed", "kitti_static"])
def test_kitti_matches_reference_gpu(trees, tmp_path, golden_dir, run):
    C.check_kitti("cuda", trees, tmp_path, golden_dir, run)


def test_cityscapes_matches_reference_gpu(trees, tmp_path, golden_dir):
    C.check_cityscapes("cuda", trees, tmp_path, golden_dir)


def test_stores_equal_stores_built_off_the_folders_gpu(trees, tmp_path, golden_dir):
    C.check_stores("cuda", trees, tmp_path, golden_dir)


def test_prepared_train_store_gives_a_finite_batch_gpu(trees, tmp_path, golden_dir):
    C.check_stores("cuda", trees, tmp_path, golden_dir, src_hw=(75, 150), hw=(64, 128), batch=True)


def test_cli_end_to_end_gpu(trees, tmp_path, golden_dir, capsys):
    C.check_cli_run("cuda", trees, tmp_path, golden_dir, capsys)


def test_greyscale_png_is_refused_by_name_gpu(tmp_path):
    C.check_grey_png("cuda", tmp_path)
