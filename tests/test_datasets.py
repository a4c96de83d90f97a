"""cc_amd.datasets on the host and on the x86 emulation build of the kernels (tests/frame_store_cases.py holds the cases; the
same ones run on the GPU in tests/test_frame_store_gpu.py): the sequence-folder crawler and its sample order against the
fixture the unmodified reference wrote (tests/golden/sequence_folder.json, tools/make_sequence_golden.py), the resident frame
store, the store-indexed transform against the host classes bit for bit, local normalisation against float64, the loader."""
import pytest

import frame_store_cases as C
from hipemu.emu import emulated_engine


@pytest.fixture(scope="module")
def emu():
    with emulated_engine():
        yield


@pytest.fixture(scope="module")
def tmp_root(tmp_path_factory):
    return tmp_path_factory.mktemp("frame_store")


def test_sequence_folder_matches_reference(tmp_path, golden_dir):
    C.check_sequence_folder(C.build_tree(tmp_path / "tree"), golden_dir)


def test_sequence_folder_rejects_other_files(tmp_path):
    C.check_bad_files(tmp_path)


def test_store_build_emulated(emu, tmp_path):
    C.check_store_build("cpu", tmp_path)


def test_store_transform_emulated(emu, tmp_root):
    C.check_store_transform("cpu", tmp_root)


def test_store_to_tensor_emulated(emu, tmp_root):
    C.check_store_to_tensor("cpu", tmp_root)


def test_local_norm_emulated(emu, tmp_root):
    C.check_local_norm("cpu", tmp_root)


def test_loader_order(emu, tmp_root):
    C.check_loader_order(C.tree_and_store("cpu", tmp_root, 36, 52, 3)[1])


def test_loader_batches_emulated(emu, tmp_root):
    C.check_loader_batches("cpu", tmp_root, 36, 52)


def test_transform_rejects_unknown_normalisation():
    from cc_amd import custom_transforms as CT
    with pytest.raises(ValueError):
        CT.DeviceTrainTransform(device="cpu", normalize="batch")
