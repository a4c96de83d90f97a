"""cc_amd.datasets.validation and metrics.flow_metrics_samples on the GPU: the cases of tests/validation_store_cases.py on the real
library, a ragged batch at KITTI 2015 sizes (the workgroup cap and the grid-stride loop), and the flow store end to end at
256 x 832."""
import pytest

import validation_store_cases as C

pytestmark = pytest.mark.gpu


def test_samples_rows_equal_single_sample_calls_gpu():
    C.check_rows_exact("cuda")


def test_samples_rows_kitti_sizes_gpu():
    """375 x 1242 and 370 x 1224 in one batch: 1820 and 1770 workgroups' worth of pixels on 512 workgroups each"""
    C.check_rows_exact("cuda", sizes=C.BIG_SIZES, pred_hw=C.BIG_PRED_HW, idx_lists=((1, 0), (0, 0)), seed=6)


def test_samples_rows_against_reference_arithmetic_gpu():
    C.check_rows_against_oracle("cuda", 2e-5)


def test_samples_meter_gpu():
    C.check_meter("cuda")


def test_samples_argument_errors_gpu():
    C.check_argument_errors("cuda")


def test_depth_store_gpu(tmp_path):
    C.check_depth_store("cuda", tmp_path)


def test_flow_store_gpu(tmp_path):
    C.check_flow_store("cuda", tmp_path)


def test_flow_store_end_to_end_kitti_size_gpu(tmp_path):
    C.check_flow_store("cuda", tmp_path, sizes=((375, 1242), (370, 1224)), hw=(256, 832), batch=2, cache=False)
