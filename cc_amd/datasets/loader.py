"""Batches for `CCTrainer.step` from a resident FrameStore: per batch the host draws the augmentation and uploads a few small
tables from pinned memory; the frames are read where they lie, nothing waits for the device."""
import numpy as np
import torch


class DeviceSequenceLoader(object):
    """Iterates (tgt [B,3,h,w], [refs ...], K [B,3,3], Kinv [B,3,3]), fp32 and contiguous on the store's device.
    Order of an epoch: torch.randperm(S) from a CPU generator seeded with seed + epoch (`set_epoch`), or arange(S); cut to a
    multiple of world_size * batch_size (drop_last=False: of world_size, and the last batch may be short); rank r takes
    order[r::world_size].  transform: a DeviceTrainTransform on the store's device.  Kinv: np.linalg.inv of the augmented float32 K,
    as the reference's loader computes it."""

    def __init__(self, store, batch_size, transform, shuffle=True, seed=0, drop_last=True, rank=0, world_size=1):
        if not 0 <= rank < world_size or batch_size < 1:
            raise ValueError("DeviceSequenceLoader: rank %d of %d, batch size %d" % (rank, world_size, batch_size))
        self.store, self.batch_size, self.transform = store, int(batch_size), transform
        self.shuffle, self.seed, self.drop_last, self.rank, self.world_size = shuffle, int(seed), drop_last, int(rank), int(world_size)
        self.epoch = 0

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def indices(self):
        """this rank's sample ids of the current epoch, in batch order"""
        S = len(self.store)
        if self.shuffle:
            order = torch.randperm(S, generator=torch.Generator().manual_seed(self.seed + self.epoch)).numpy()
        else:
            order = np.arange(S)
        group = self.world_size * (self.batch_size if self.drop_last else 1)
        return order[:S // group * group][self.rank::self.world_size]

    def __len__(self):
        n = len(self.indices())
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def __iter__(self):
        ids = self.indices()
        dev = self.store.device
        for i in range(len(self)):
            x, Ks = self.transform.from_store(self.store, ids[i * self.batch_size:(i + 1) * self.batch_size], frame_major=True)
            K = np.stack([np.asarray(k, dtype=np.float32) for k in Ks])
            KK = torch.from_numpy(np.stack([K, np.stack([np.linalg.inv(k) for k in K])]))
            if dev.type == "cuda":
                KK = KK.pin_memory()
            KK = KK.to(dev, non_blocking=True)
            yield x[0], [x[j] for j in range(1, x.shape[0])], KK[0], KK[1]
