"""The training set resident in HBM: every distinct frame decoded once (Pillow, on the host, in a thread pool) and kept as uint8,
with the per-frame (min, max) the reference's resize / rotate byte-scale by, the scenes' intrinsics and the samples as frame ids.
F frames of H x W take F * H * W * 3 + 8 F bytes of device memory (`nbytes`)."""
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .._lib import engine, STREAM
from .sequence_folders import crawl, load_as_uint8

FORMAT = 1
HEADER = "store.json"


class _Uploader(object):
    """Host frames -> frames[lo:hi] on the device through two reused staging buffers (pinned when the store lives on a HIP
    device).  The copy out of a buffer is asynchronous; an event per buffer says when it has completed, and a buffer is not
    refilled before that.  Each uploaded range gets its (min, max) rows from cc_store_minmax, behind its copy on the stream."""

    def __init__(self, frames, minmax, chunk_frames):
        self.frames, self.minmax = frames, minmax
        self.cuda = frames.is_cuda
        self.chunk = max(1, int(chunk_frames))
        shape = (self.chunk,) + tuple(frames.shape[1:])
        self.bufs = [torch.empty(shape, dtype=torch.uint8, pin_memory=self.cuda) for _ in range(2)]
        self.events = [None, None]

    def run(self, fill, with_minmax=True):
        """fill(lo, hi, out): write frames lo..hi-1 into the numpy view out [hi-lo,H,W,3]."""
        F = self.frames.shape[0]
        per_frame = int(np.prod(self.frames.shape[1:]))
        for k, lo in enumerate(range(0, F, self.chunk)):
            hi, b = min(F, lo + self.chunk), k % 2
            if self.events[b] is not None:
                self.events[b].synchronize()                 # the copy that last read this buffer has completed
            fill(lo, hi, self.bufs[b].numpy()[:hi - lo])
            self.frames[lo:hi].copy_(self.bufs[b][:hi - lo], non_blocking=True)
            if self.cuda:
                self.events[b] = torch.cuda.Event()
                self.events[b].record()
            if with_minmax:
                engine().call("cc_store_minmax", self.frames[lo:hi], self.minmax[lo:hi], hi - lo, per_frame, STREAM)
        if self.cuda:
            torch.cuda.current_stream().synchronize()        # the staging buffers are released with this object


def frame_tables(found):
    """crawl's samples -> (paths: each distinct frame once, in order of first use; samples int32 [S,1+R] of ids into paths;
    sample_scene int32 [S]) -- the store's frame order, shared with the stores `datasets.prepare` writes directly"""
    ids, paths = {}, []
    for _, ps in found:
        for p in ps:
            if p not in ids:
                ids[p] = len(paths)
                paths.append(p)
    samples = np.array([[ids[p] for p in ps] for _, ps in found], dtype=np.int32)
    sample_scene = np.array([s for s, _ in found], dtype=np.int32)
    return paths, samples, sample_scene


class FrameStore(object):
    """frames: uint8 [F,H,W,3] on the device, each distinct frame once; minmax: fp32 [F,2] on the device.  On the host (the batch
    tables are drawn there): intrinsics float32 [scenes,3,3]; samples int32 [S,1+R], frame ids with the target first and the
    references in the order -d .. -1, +1 .. +d; sample_scene int32 [S], each sample's row of intrinsics; scenes: their names."""

    def __init__(self, frames, minmax, intrinsics, samples, sample_scene, scenes):
        self.frames, self.minmax = frames, minmax
        self.intrinsics = torch.as_tensor(intrinsics, dtype=torch.float32).contiguous()
        self.samples = torch.as_tensor(samples, dtype=torch.int32).contiguous()
        self.sample_scene = torch.as_tensor(sample_scene, dtype=torch.int32).contiguous()
        self.scenes = list(scenes)
        self.intrinsics_np, self.samples_np, self.sample_scene_np = self.intrinsics.numpy(), self.samples.numpy(), self.sample_scene.numpy()
        F, S = int(frames.shape[0]), int(self.samples.shape[0])
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or tuple(minmax.shape) != (F, 2) or \
                minmax.dtype != torch.float32 or self.samples.dim() != 2 or tuple(self.sample_scene.shape) != (S,) or \
                tuple(self.intrinsics.shape) != (len(self.scenes), 3, 3):
            raise ValueError("FrameStore: arrays of inconsistent shapes / types")
        if S and (int(self.samples_np.min()) < 0 or int(self.samples_np.max()) >= F or int(self.sample_scene_np.min()) < 0 or
                  int(self.sample_scene_np.max()) >= len(self.scenes)):
            raise ValueError("FrameStore: a sample names a frame or a scene outside the store")

    @property
    def device(self):
        return self.frames.device

    @property
    def nbytes(self):
        """device bytes: F * H * W * 3 + 8 F"""
        return self.frames.numel() + self.minmax.numel() * 4

    def __len__(self):
        return int(self.samples.shape[0])

    @classmethod
    def build(cls, root, train=True, sequence_length=5, device="cuda", workers=8, chunk_frames=256, max_bytes=None):
        scenes, intrinsics, found = crawl(root, train, sequence_length)
        if not found:
            raise ValueError("%s: no scene with %d or more frames" % (root, sequence_length))
        paths, samples, sample_scene = frame_tables(found)
        first = load_as_uint8(paths[0])
        H, W, F = first.shape[0], first.shape[1], len(paths)
        total = F * H * W * 3 + 8 * F
        if max_bytes is not None and total > max_bytes:
            raise ValueError("%s: %d frames of %d x %d need %d bytes, more than max_bytes = %d" % (root, F, H, W, total, max_bytes))
        device = torch.device(device)
        frames = torch.empty((F, H, W, 3), dtype=torch.uint8, device=device)
        minmax = torch.empty((F, 2), dtype=torch.float32, device=device)

        def decode(job):
            path, out = job
            a = load_as_uint8(path)
            if a.shape != out.shape:
                raise ValueError("%s: %d x %d, the store's frames are %d x %d" % (path, a.shape[0], a.shape[1], H, W))
            out[...] = a

        with ThreadPoolExecutor(max_workers=max(1, int(workers))) as pool:
            _Uploader(frames, minmax, chunk_frames).run(lambda lo, hi, out: list(pool.map(decode, [(paths[i], out[i - lo]) for i in range(lo, hi)])))
        return cls(frames, minmax, intrinsics, samples, sample_scene, scenes)

    # ---- the store's own cache: .npy files + a small JSON header
    def _header(self):
        F, H, W, _ = self.frames.shape
        return {"format": FORMAT, "frames": [int(F), int(H), int(W), 3], "samples": [int(v) for v in self.samples.shape],
                "scenes": self.scenes, "nbytes": int(self.nbytes)}

    def save(self, directory, chunk_frames=256):
        from numpy.lib.format import open_memmap
        os.makedirs(directory, exist_ok=True)
        F = int(self.frames.shape[0])
        mm = open_memmap(os.path.join(directory, "frames.npy"), mode="w+", dtype=np.uint8, shape=tuple(self.frames.shape))
        for lo in range(0, F, chunk_frames):
            mm[lo:lo + chunk_frames] = self.frames[lo:lo + chunk_frames].cpu().numpy()
        mm.flush()
        del mm
        np.save(os.path.join(directory, "minmax.npy"), self.minmax.cpu().numpy())
        np.save(os.path.join(directory, "intrinsics.npy"), self.intrinsics_np)
        np.save(os.path.join(directory, "samples.npy"), self.samples_np)
        np.save(os.path.join(directory, "sample_scene.npy"), self.sample_scene_np)
        with open(os.path.join(directory, HEADER), "w") as f:
            json.dump(self._header(), f, indent=1)

    @classmethod
    def load(cls, directory, device="cuda", chunk_frames=256):
        with open(os.path.join(directory, HEADER)) as f:
            hdr = json.load(f)
        if hdr.get("format") != FORMAT:
            raise ValueError("%s: store format %r, this build reads %d" % (directory, hdr.get("format"), FORMAT))
        src = np.load(os.path.join(directory, "frames.npy"), mmap_mode="r")
        arrays = {n: np.load(os.path.join(directory, n + ".npy")) for n in ("minmax", "intrinsics", "samples", "sample_scene")}
        F = src.shape[0]
        want = {"frames": (tuple(hdr["frames"]), np.uint8, src), "minmax": ((F, 2), np.float32, arrays["minmax"]),
                "intrinsics": ((len(hdr["scenes"]), 3, 3), np.float32, arrays["intrinsics"]),
                "samples": (tuple(hdr["samples"]), np.int32, arrays["samples"]),
                "sample_scene": ((hdr["samples"][0],), np.int32, arrays["sample_scene"])}
        for name, (shape, dtype, a) in want.items():
            if tuple(a.shape) != tuple(shape) or a.dtype != dtype:
                raise ValueError("%s: %s.npy is %s %s, the header says %s %s" % (directory, name, a.dtype, a.shape, np.dtype(dtype), shape))
        if hdr["nbytes"] != src.size + 8 * F:
            raise ValueError("%s: the header's nbytes does not match its frames" % directory)
        device = torch.device(device)
        frames = torch.empty(src.shape, dtype=torch.uint8, device=device)
        minmax = torch.from_numpy(arrays["minmax"]).to(device)

        def fill(lo, hi, out):
            out[...] = src[lo:hi]

        _Uploader(frames, minmax, chunk_frames).run(fill, with_minmax=False)
        return cls(frames, minmax, arrays["intrinsics"], arrays["samples"], arrays["sample_scene"], hdr["scenes"])
