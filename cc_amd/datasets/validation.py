"""The validation sets (the reference's datasets/validation_folders.py and, through cc_amd.kitti_eval.Kitti2015Flow, its
datasets/validation_flow.py) and their device-resident forms.

`ValidationSet`: the depth validation folder on the host, in the reference's order.  `DepthValStore` + `DeviceDepthValLoader`: its
frames (uint8) and depth maps (fp32) in HBM, handed out as the batches `validate_depth_with_gt` takes.  `FlowValStore` +
`DeviceFlowValLoader`: the KITTI 2015 flow samples in HBM -- the network inputs as the loader would hand them over, the intrinsics,
and the decoded flow ground truth and object maps of all sizes in two fp32 pools described by an offset table, which is what
`metrics.flow_metrics_samples` scores a ragged batch from."""
import fnmatch
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
import torch.utils.data as data

from .frame_store import _Uploader
from .sequence_folders import load_as_float, load_as_uint8

FORMAT = 1
HEADER = "store.json"


def crawl_validation(root):
    """-> (scenes, imgs, depth): the scene names of val.txt in file order (a last line without a newline counts), every scene's
    sorted `*.jpg` and the `.npy` beside each.  A frame without its depth file raises FileNotFoundError."""
    with open(os.path.join(root, "val.txt")) as f:
        scenes = [line.rstrip("\n") for line in f if line.strip()]
    imgs, depth = [], []
    for name in scenes:
        folder = os.path.join(root, name)
        for img in sorted(os.path.join(folder, n) for n in os.listdir(folder)
                          if fnmatch.fnmatchcase(n, "*.jpg") and os.path.isfile(os.path.join(folder, n))):
            d = img[:-4] + ".npy"
            if not os.path.isfile(d):
                raise FileNotFoundError("depth file %s not found" % d)
            imgs.append(img)
            depth.append(d)
    return scenes, imgs, depth


class ValidationSet(data.Dataset):
    """root/scene_1/0000000.jpg, root/scene_1/0000000.npy, root/scene_1/0000001.jpg, ..., the scenes named by root/val.txt.
    transform: takes a list of images and None.  -> (img, depth) per frame: float32 HWC (or what the transform makes of it) and the
    float32 depth map."""

    def __init__(self, root, transform=None):
        self.root = root
        self.scenes, self.imgs, self.depth = crawl_validation(root)
        self.transform = transform

    def __getitem__(self, index):
        img = load_as_float(self.imgs[index])
        depth = np.load(self.depth[index]).astype(np.float32)
        if self.transform is not None:
            img, _ = self.transform([img], None)
            img = img[0]
        return img, depth

    def __len__(self):
        return len(self.imgs)


def _check_header(directory, kind):
    with open(os.path.join(directory, HEADER)) as f:
        hdr = json.load(f)
    if hdr.get("format") != FORMAT or hdr.get("kind") != kind:
        raise ValueError("%s: store format %r of kind %r, this build reads format %d of kind %r"
                         % (directory, hdr.get("format"), hdr.get("kind"), FORMAT, kind))
    return hdr


def _load_arrays(directory, want):
    """want: {name: (shape, dtype)} -> {name: array} (memory-mapped), each checked against the header's word"""
    out = {}
    for name, (shape, dtype) in want.items():
        a = np.load(os.path.join(directory, name + ".npy"), mmap_mode="r")
        if tuple(a.shape) != tuple(shape) or a.dtype != dtype:
            raise ValueError("%s: %s.npy is %s %s, the header says %s %s" % (directory, name, a.dtype, a.shape, np.dtype(dtype), tuple(shape)))
        out[name] = a
    return out


def _save_chunked(path, t, chunk):
    from numpy.lib.format import open_memmap
    mm = open_memmap(path, mode="w+", dtype=np.dtype(str(t.dtype).replace("torch.", "")), shape=tuple(t.shape))
    for lo in range(0, t.shape[0], chunk):
        mm[lo:lo + chunk] = t[lo:lo + chunk].cpu().numpy()
    mm.flush()
    del mm


class DepthValStore(object):
    """frames: uint8 [F,H,W,3] and depth: fp32 [F,Hd,Wd], both on the device, in `ValidationSet` order; names: the frames' paths
    relative to the root, on the host.  F * H * W * 3 + 4 F * Hd * Wd bytes of device memory (`nbytes`)."""

    def __init__(self, frames, depth, names):
        self.frames, self.depth, self.names = frames, depth, list(names)
        F = int(frames.shape[0])
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or depth.dtype != torch.float32 or depth.dim() != 3 or \
                depth.shape[0] != F or len(self.names) != F or depth.device != frames.device:
            raise ValueError("DepthValStore: arrays of inconsistent shapes / types")

    @property
    def device(self):
        return self.frames.device

    @property
    def nbytes(self):
        return self.frames.numel() + 4 * self.depth.numel()

    def __len__(self):
        return int(self.frames.shape[0])

    @classmethod
    def build(cls, root, device="cuda", workers=8, max_bytes=None, chunk_frames=256):
        _, imgs, depths = crawl_validation(root)
        if not imgs:
            raise ValueError("%s: no validation frame" % root)
        first = load_as_uint8(imgs[0])
        H, W, F = first.shape[0], first.shape[1], len(imgs)
        dshape = tuple(np.load(depths[0], mmap_mode="r").shape)
        if len(dshape) != 2:
            raise ValueError("%s: a depth map of shape %s" % (depths[0], dshape))
        Hd, Wd = dshape
        total = F * H * W * 3 + 4 * F * Hd * Wd
        if max_bytes is not None and total > max_bytes:
            raise ValueError("%s: %d frames of %d x %d with depth maps of %d x %d need %d bytes, more than max_bytes = %d"
                             % (root, F, H, W, Hd, Wd, total, max_bytes))
        device = torch.device(device)
        frames = torch.empty((F, H, W, 3), dtype=torch.uint8, device=device)
        depth = torch.empty((F, Hd, Wd), dtype=torch.float32, device=device)

        def decode(job):
            path, out = job
            a = load_as_uint8(path)
            if a.shape != out.shape:
                raise ValueError("%s: %d x %d, the store's frames are %d x %d" % (path, a.shape[0], a.shape[1], H, W))
            out[...] = a

        def read_depth(job):
            path, out = job
            a = np.load(path)
            if a.shape != (Hd, Wd):
                raise ValueError("%s: a depth map of shape %s, the store's are %d x %d" % (path, tuple(a.shape), Hd, Wd))
            out.view(np.float32)[...] = a.astype(np.float32)

        with ThreadPoolExecutor(max_workers=max(1, int(workers))) as pool:
            _Uploader(frames, None, chunk_frames).run(
                lambda lo, hi, out: list(pool.map(decode, [(imgs[i], out[i - lo]) for i in range(lo, hi)])), with_minmax=False)
            # the depth maps through the same staging buffers, as the bytes of their floats
            _Uploader(depth.view(torch.uint8), None, chunk_frames).run(
                lambda lo, hi, out: list(pool.map(read_depth, [(depths[i], out[i - lo]) for i in range(lo, hi)])), with_minmax=False)
        return cls(frames, depth, [os.path.relpath(p, str(root)).replace(os.sep, "/") for p in imgs])

    def save(self, directory, chunk_frames=256):
        os.makedirs(directory, exist_ok=True)
        _save_chunked(os.path.join(directory, "frames.npy"), self.frames, chunk_frames)
        _save_chunked(os.path.join(directory, "depth.npy"), self.depth, chunk_frames)
        with open(os.path.join(directory, HEADER), "w") as f:
            json.dump({"format": FORMAT, "kind": "depth_val", "frames": [int(v) for v in self.frames.shape],
                       "depth": [int(v) for v in self.depth.shape], "names": self.names, "nbytes": int(self.nbytes)}, f, indent=1)

    @classmethod
    def load(cls, directory, device="cuda", chunk_frames=256):
        hdr = _check_header(directory, "depth_val")
        a = _load_arrays(directory, {"frames": (hdr["frames"], np.uint8), "depth": (hdr["depth"], np.float32)})
        src, dsrc = a["frames"], a["depth"]
        if len(hdr["frames"]) != 4 or len(hdr["depth"]) != 3 or hdr["depth"][0] != hdr["frames"][0] or len(hdr["names"]) != hdr["frames"][0] \
                or hdr["nbytes"] != src.size + 4 * dsrc.size:
            raise ValueError("%s: the header does not match its arrays" % directory)
        device = torch.device(device)
        frames = torch.empty(src.shape, dtype=torch.uint8, device=device)
        depth = torch.empty(dsrc.shape, dtype=torch.float32, device=device)

        def fill(lo, hi, out):
            out[...] = src[lo:hi]

        def fill_depth(lo, hi, out):
            out.view(np.float32)[...] = dsrc[lo:hi]

        _Uploader(frames, None, chunk_frames).run(fill, with_minmax=False)
        _Uploader(depth.view(torch.uint8), None, chunk_frames).run(fill_depth, with_minmax=False)
        return cls(frames, depth, hdr["names"])


class DeviceDepthValLoader(object):
    """Iterates (tgt_img [b,3,H,W], depth [b,Hd,Wd]) on the store's device, in the store's order; the last batch may be short.
    These are, bit for bit, the batches of DataLoader(ValidationSet(root, Compose([ArrayToTensor(), Normalize(mean, std)])),
    batch_size, shuffle=False); the frames go through DeviceFrames.store_to_tensor."""

    def __init__(self, store, batch_size, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5)):
        from ..custom_transforms import DeviceFrames
        if batch_size < 1:
            raise ValueError("DeviceDepthValLoader: batch size %d" % batch_size)
        self.store, self.batch_size = store, int(batch_size)
        self.prep = DeviceFrames(mean, std, device=store.device)

    def __len__(self):
        return -(-len(self.store) // self.batch_size)

    def __iter__(self):
        F = len(self.store)
        for lo in range(0, F, self.batch_size):
            hi = min(F, lo + self.batch_size)
            yield self.prep.store_to_tensor(self.store, np.arange(lo, hi, dtype=np.int32)), self.store.depth[lo:hi]


def _png_size(path):
    """(H, W) from the IHDR chunk of a PNG file"""
    import struct
    with open(str(path), "rb") as f:
        head = f.read(24)
    if len(head) < 24 or head[:8] != b'\x89PNG\r\n\x1a\n' or head[12:16] != b'IHDR':
        raise ValueError("%s: not a PNG file" % path)
    W, H = struct.unpack(">II", head[16:24])
    return int(H), int(W)


class FlowValStore(object):
    """A Kitti2015Flow framework resident on the device, for `validate.validate_flow_from_store`.  Per sample:
      inputs      fp32 [1+R,n,3,h,w] (frame-major: inputs[j, lo:hi] is a contiguous batch) -- the target and the R reference frames
                  as `kitti_eval.kitti2015_item` hands them to the loop, computed once through it, so identical by construction;
      K, Kinv     fp32 [n,3,3], the scaled intrinsics and their inverse, from the same call;
      flow_pool   fp32, the decoded (u, v, valid) ground truth [3,Hg,Wg] of every sample, each at its own size;
      obj_pool    fp32, the object maps [Hg,Wg];
      table       int64 [n,4] rows {flow offset, obj-map offset, Hg, Wg} (offsets in floats), on the host (`table_np`) and on
                  the device; rows [n] int32 = arange(n) on the device (a batch's `idx` is a slice of it); max_px: max Hg * Wg.
    For KITTI 2015 at 256 x 832 a sample takes 5 * 3 * 256 * 832 * 4 B = 12.8 MB of inputs and, at 375 x 1242, 4 * 375 * 1242 * 4 B
    = 7.5 MB of ground truth: about 4 GB for the 200 samples (`nbytes`)."""

    def __init__(self, inputs, K, Kinv, flow_pool, obj_pool, table):
        self.inputs, self.K, self.Kinv, self.flow_pool, self.obj_pool = inputs, K, Kinv, flow_pool, obj_pool
        self.table_np = np.ascontiguousarray(table, dtype=np.int64)
        n = int(inputs.shape[1]) if inputs.dim() == 5 else -1
        if inputs.dim() != 5 or inputs.shape[2] != 3 or inputs.dtype != torch.float32 or tuple(K.shape) != (n, 3, 3) or \
                tuple(Kinv.shape) != (n, 3, 3) or flow_pool.dim() != 1 or obj_pool.dim() != 1 or flow_pool.dtype != torch.float32 or \
                obj_pool.dtype != torch.float32 or self.table_np.shape != (n, 4) or n < 1:
            raise ValueError("FlowValStore: arrays of inconsistent shapes / types")
        t = self.table_np
        px = t[:, 2] * t[:, 3]
        if (t[:, 2:] <= 0).any() or (t[:, :2] < 0).any() or (t[:, 0] + 3 * px > flow_pool.numel()).any() or \
                (t[:, 1] + px > obj_pool.numel()).any():
            raise ValueError("FlowValStore: a table row reaches outside the pools")
        self.max_px = int(px.max())
        dev = inputs.device
        self.table = torch.from_numpy(self.table_np).to(dev)
        self.rows = torch.arange(n, dtype=torch.int32, device=dev)
        self._gt_nan = None

    @property
    def device(self):
        return self.inputs.device

    @property
    def nbytes(self):
        return 4 * (self.inputs.numel() + self.K.numel() + self.Kinv.numel() + self.flow_pool.numel() + self.obj_pool.numel()) + \
            8 * self.table.numel() + 4 * self.rows.numel()

    def __len__(self):
        return int(self.inputs.shape[1])

    def flow_gt(self, i):
        """[1,3,Hg,Wg], a view of the pool"""
        fo, _, Hg, Wg = (int(v) for v in self.table_np[i])
        return self.flow_pool[fo:fo + 3 * Hg * Wg].view(1, 3, Hg, Wg)

    def obj_map(self, i):
        """[1,Hg,Wg], a view of the pool"""
        _, oo, Hg, Wg = (int(v) for v in self.table_np[i])
        return self.obj_pool[oo:oo + Hg * Wg].view(1, Hg, Wg)

    def gt_nan(self):
        """device flag: a NaN in the flow ground truth (the first half of train.py:746), computed once"""
        if self._gt_nan is None:
            self._gt_nan = torch.isnan(self.flow_pool.sum())
        return self._gt_nan

    @classmethod
    def build(cls, framework, img_hw, device="cuda", max_bytes=None):
        from ..custom_transforms import DeviceFrames
        from ..kitti_eval import kitti2015_item
        n, R = len(framework), len(framework.seq_ids)
        h, w = (int(v) for v in img_hw)
        sizes = [_png_size(framework.paths(i)['flow']) for i in range(n)]
        px = np.array([Hg * Wg for Hg, Wg in sizes], dtype=np.int64)
        table = np.zeros((n, 4), dtype=np.int64)
        table[:, 0] = np.concatenate([[0], np.cumsum(3 * px)[:-1]])
        table[:, 1] = np.concatenate([[0], np.cumsum(px)[:-1]])
        table[:, 2:] = np.array(sizes, dtype=np.int64)
        total = 4 * (n * (1 + R) * 3 * h * w + 18 * n + 4 * int(px.sum())) + 36 * n
        if max_bytes is not None and total > max_bytes:
            raise ValueError("%d samples at %d x %d with %d ground-truth pixels need %d bytes, more than max_bytes = %d"
                             % (n, h, w, int(px.sum()), total, max_bytes))
        device = torch.device(device)
        frames_dev = DeviceFrames(device=device)
        inputs = torch.empty((1 + R, n, 3, h, w), dtype=torch.float32, device=device)
        K = torch.empty((n, 3, 3), dtype=torch.float32, device=device)
        Kinv = torch.empty((n, 3, 3), dtype=torch.float32, device=device)
        flow_pool = torch.empty(3 * int(px.sum()), dtype=torch.float32, device=device)
        obj_pool = torch.empty(int(px.sum()), dtype=torch.float32, device=device)
        for i in range(n):
            tgt, refs, Ki, Kinvi, flow_gt, obj, _ = kitti2015_item(framework[i], (h, w), frames_dev)
            Hg, Wg = sizes[i]
            if tuple(flow_gt.shape) != (1, 3, Hg, Wg) or tuple(obj.shape) != (1, Hg, Wg) or len(refs) != R:
                raise ValueError("sample %d: flow ground truth %s and object map %s, the flow file's header says %d x %d"
                                 % (i, tuple(flow_gt.shape), tuple(obj.shape), Hg, Wg))
            inputs[0, i] = tgt[0]
            for j, r in enumerate(refs):
                inputs[1 + j, i] = r[0]
            K[i], Kinv[i] = Ki[0], Kinvi[0]
            flow_pool[table[i, 0]:table[i, 0] + 3 * px[i]] = flow_gt.reshape(-1)
            obj_pool[table[i, 1]:table[i, 1] + px[i]] = obj.reshape(-1)
        return cls(inputs, K, Kinv, flow_pool, obj_pool, table)

    def save(self, directory, chunk=1 << 24):
        os.makedirs(directory, exist_ok=True)
        _save_chunked(os.path.join(directory, "inputs.npy"), self.inputs, 1)
        for name in ("K", "Kinv"):
            np.save(os.path.join(directory, name + ".npy"), getattr(self, name).cpu().numpy())
        _save_chunked(os.path.join(directory, "flow_pool.npy"), self.flow_pool, chunk)
        _save_chunked(os.path.join(directory, "obj_pool.npy"), self.obj_pool, chunk)
        np.save(os.path.join(directory, "table.npy"), self.table_np)
        with open(os.path.join(directory, HEADER), "w") as f:
            json.dump({"format": FORMAT, "kind": "flow_val", "inputs": [int(v) for v in self.inputs.shape],
                       "flow_floats": int(self.flow_pool.numel()), "obj_floats": int(self.obj_pool.numel()),
                       "nbytes": int(self.nbytes)}, f, indent=1)

    @classmethod
    def load(cls, directory, device="cuda", chunk=1 << 24):
        hdr = _check_header(directory, "flow_val")
        if len(hdr["inputs"]) != 5:
            raise ValueError("%s: the header's inputs are not [1+R,n,3,h,w]" % directory)
        n = hdr["inputs"][1]
        a = _load_arrays(directory, {"inputs": (hdr["inputs"], np.float32), "K": ((n, 3, 3), np.float32), "Kinv": ((n, 3, 3), np.float32),
                                     "flow_pool": ((hdr["flow_floats"],), np.float32), "obj_pool": ((hdr["obj_floats"],), np.float32),
                                     "table": ((n, 4), np.int64)})
        device = torch.device(device)

        def upload(src, step):
            dst = torch.empty(src.shape, dtype=torch.float32, device=device)
            for lo in range(0, src.shape[0], step):
                dst[lo:lo + step] = torch.from_numpy(np.array(src[lo:lo + step])).to(device)
            return dst

        store = cls(upload(a["inputs"], 1), upload(a["K"], n), upload(a["Kinv"], n), upload(a["flow_pool"], chunk),
                    upload(a["obj_pool"], chunk), np.array(a["table"]))
        if hdr["nbytes"] != store.nbytes:
            raise ValueError("%s: the header's nbytes does not match its arrays" % directory)
        return store


class DeviceFlowValLoader(object):
    """A FlowValStore in its own order, never shuffled.  Iterating (batch size 1 only) yields the six-tuple of
    `validate_flow_with_gt`: (tgt_img [1,3,h,w], ref_imgs, intrinsics [1,3,3], intrinsics_inv, flow_gt [1,3,Hg,Wg], obj_map_gt
    [1,Hg,Wg]), views of the store.  `batches()` yields, at any batch size, (tgt [b,3,h,w], refs, K [b,3,3], Kinv, idx int32 [b])
    for the batched loop, which scores the ground truth through the store's table; the last batch may be short."""

    def __init__(self, store, batch_size=1):
        if batch_size < 1:
            raise ValueError("DeviceFlowValLoader: batch size %d" % batch_size)
        self.store, self.batch_size = store, int(batch_size)

    def __len__(self):
        return -(-len(self.store) // self.batch_size)

    def batches(self):
        s = self.store
        for lo in range(0, len(s), self.batch_size):
            hi = min(len(s), lo + self.batch_size)
            yield s.inputs[0, lo:hi], [s.inputs[j, lo:hi] for j in range(1, s.inputs.shape[0])], s.K[lo:hi], s.Kinv[lo:hi], s.rows[lo:hi]

    def __iter__(self):
        if self.batch_size != 1:
            raise ValueError("DeviceFlowValLoader: the ground truths differ in size, so the six-tuples come one sample at a time; "
                             "use batches() at batch size %d" % self.batch_size)
        for i, (tgt, refs, K, Kinv, _) in enumerate(self.batches()):
            yield tgt, refs, K, Kinv, self.store.flow_gt(i), self.store.obj_map(i)
