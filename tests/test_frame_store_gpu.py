"""cc_amd.datasets on the GPU: the cases of tests/frame_store_cases.py on the real library, at the emulator's sizes and at
128 x 416; frame offsets beyond 4 GiB; three captured training steps fed by the loader."""
import random

import numpy as np
import pytest
import torch

import frame_store_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tmp_root(tmp_path_factory):
    return tmp_path_factory.mktemp("frame_store_gpu")


def test_store_build_gpu(tmp_path):
    C.check_store_build("cuda", tmp_path)


def test_store_transform_gpu(tmp_root):
    C.check_store_transform("cuda", tmp_root, sizes=((40, 56), (36, 52), (128, 416)))


def test_store_to_tensor_gpu(tmp_root):
    C.check_store_to_tensor("cuda", tmp_root)


def test_local_norm_gpu(tmp_root):
    C.check_local_norm("cuda", tmp_root, sizes=((36, 52), (128, 416)))


def test_store_beyond_4gib():
    """A store of 6 800 frames of 256 x 832 x 3 (4.34 GB, left uninitialised) with real frames at ids 0 and 6 799: the transform of
    ids [6799, 0] equals the transform of a two-frame store that holds the same frames -- the last frame starts 4.34e9 bytes into
    the store, past what a 32-bit offset reaches."""
    from cc_amd import custom_transforms as CT, datasets as DS
    F, H, W = 6800, 256, 832
    assert (F - 1) * H * W * 3 > 2 ** 32
    dev = torch.device("cuda")
    r = np.random.RandomState(4)
    two = torch.from_numpy((40 + r.rand(2, H, W, 3) * 180).astype(np.uint8)).to(dev)
    mm2 = torch.stack([two.view(2, -1).min(1).values, two.view(2, -1).max(1).values], 1).float()
    big = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
    mm = torch.empty((F, 2), dtype=torch.float32, device=dev)
    big[0], big[F - 1], mm[0], mm[F - 1] = two[0], two[1], mm2[0], mm2[1]
    K = C.scene_intrinsics(0, H, W)[None]
    large = DS.FrameStore(big, mm, K, [[F - 1], [0]], [0, 0], ["s"])
    small = DS.FrameStore(two, mm2, K, [[1], [0]], [0, 0], ["s"])
    got = torch.empty((2, 2), dtype=torch.float32, device=dev)
    from cc_amd._lib import engine, STREAM
    engine().call("cc_store_minmax", big[F - 1:], got[1:], 1, H * W * 3, STREAM)        # the last frame's row, computed in place
    engine().call("cc_store_minmax", big[:1], got[:1], 1, H * W * 3, STREAM)
    assert torch.equal(got, mm2)
    for rotate in (False, True):
        tr = CT.DeviceTrainTransform(C.MEAN, C.STD, device=dev, rotate=rotate)
        outs = []
        for store in (large, small):
            random.seed(11)
            np.random.seed(11)
            outs.append(tr.from_store(store, [0, 1]))
        assert torch.equal(outs[0][0], outs[1][0]) and float(outs[1][0].std()) > 0.1
        assert all(np.array_equal(a, b) for a, b in zip(outs[0][1], outs[1][1]))
    plain = CT.DeviceFrames(device=dev)
    assert torch.equal(plain.store_to_tensor(large, [F - 1, 0]), plain.store_to_tensor(small, [1, 0]))


def test_loader_feeds_the_captured_step(tmp_root):
    """Three consecutive loader batches (B = 2, 64 x 128) through a fresh CCTrainer's captured step, on seeded weights; every batch
    equals the host pipeline's."""
    from cc_amd import trainer as T, synthetic as syn
    dev = torch.device("cuda")
    nets = T.build_nets(dev, init=False)
    for n in nets:
        n.load_state_dict(syn.seeded_state_dict(n, 0))
    tr = T.CCTrainer(nets, T.StepConfig(), use_graph=True)
    losses = []

    def step(batch):
        losses.append({k: v.clone() for k, v in tr.step(batch).items()})

    C.check_loader_batches("cuda", tmp_root, 64, 128, B=2, step=step, n_batches=3)
    tr.check_finite()
    assert len(losses) == 3 and all(bool(torch.isfinite(v).all()) for l in losses for v in l.values())
    assert any(not torch.equal(losses[0][k], losses[2][k]) for k in losses[0])      # the batches reached the step
