"""From a KITTI raw or Cityscapes download to the sequence folders `FrameStore.build` and `cc_amd.train` read: the reference's
data/prepare_train_data.py with kitti_raw_loader.py and cityscapes_loader.py, restated on the current stack (their
`scipy.misc.imread / imresize / imsave`, `np.int` and `path.Path` are gone).

`KittiRaw` and `Cityscapes` restate the two loaders' metadata code: which drives / cities, which frames, which intrinsics.  They
read no pixel beyond the size of one frame.  `prepare` does the work per scene: host threads decode the PNGs (Pillow), one pinned
upload per chunk, `cc_frames_resize_u8` (Pillow's 8-bit bilinear resample, bit for bit, cc_amd/csrc/prep_raw.hip), with get_gt
`kitti_eval.velo_depth` per kept frame, the frames back to the host where Pillow writes `<rel_path>/<frame>.jpg` -- then `cam.txt`,
`<frame>.npy`, and the train / val split of prepare_train_data.py:78-89.  With `store_cache` the resized frames, still on the
device, also become the caches `cc_amd.train --store-cache` loads.

Where this departs from the reference ("Data preparation"): the scene folders are split in sorted order (the
reference takes them in directory order); the KITTI test-scene list is passed by the caller; a frame that is not an 8-bit RGB PNG
raises ValueError; the direct stores hold the resized frames themselves, never JPEG-coded."""
import fnmatch
import json
import os
import shutil
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .._lib import engine, STREAM
from ..custom_transforms import resample_table
from ..kitti_eval import PNG_SIGNATURE, velo_depth
from .frame_store import FrameStore, frame_tables
from .sequence_folders import crawl
from .validation import DepthValStore, crawl_validation

SPLIT_SEED = 8964                                                        # prepare_train_data.py:78
CAM_FORMAT = '%f,0.,%f,0.,%f,%f,0.,0.,1.'                                # prepare_train_data.py:39
STAGES = ("crawl", "decode", "upload", "resize", "depth", "download", "encode", "split", "stores")


def _dirs(folder):
    """the sub-directories of `folder`, sorted; none where it does not exist"""
    if not os.path.isdir(folder):
        return []
    return sorted(os.path.join(folder, n) for n in os.listdir(folder) if os.path.isdir(os.path.join(folder, n)))


def _files(folder, pattern):
    if not os.path.isdir(folder):
        return []
    return sorted(os.path.join(folder, n) for n in os.listdir(folder)
                  if fnmatch.fnmatchcase(n, pattern) and os.path.isfile(os.path.join(folder, n)))


def _lines(path_or_list):
    if isinstance(path_or_list, (str, os.PathLike)):
        with open(path_or_list) as f:
            return [line.rstrip("\n") for line in f]
    return [str(v) for v in path_or_list]


def load_png_rgb8(path):
    """One 8-bit RGB PNG -> uint8 [H,W,3]; ValueError naming the file for anything else (greyscale, palette, 16 bits, alpha,
    another format, not an image) -- `load_as_uint8`'s rule for the JPEGs, applied to the downloads."""
    from PIL import Image, UnidentifiedImageError
    with open(path, "rb") as f:
        head = f.read(26)
    if len(head) < 26 or head[:8] != PNG_SIGNATURE or head[12:16] != b'IHDR':
        raise ValueError("%s: expected an 8-bit RGB PNG, found no PNG header" % path)
    if (head[24], head[25]) != (8, 2):
        raise ValueError("%s: expected an 8-bit RGB PNG, found bit depth %d / colour type %d" % (path, head[24], head[25]))
    try:
        with Image.open(path) as im:
            if im.mode != "RGB":
                raise ValueError("%s: expected an 8-bit RGB PNG, found mode %s" % (path, im.mode))
            return np.asarray(im)
    except UnidentifiedImageError as e:
        raise ValueError("%s: not an image (%s)" % (path, e))


def image_size(path):
    """(H, W) of an image file, from its header"""
    from PIL import Image
    with Image.open(path) as im:
        return im.size[1], im.size[0]


def read_raw_calib_file(path):
    """kitti_raw_loader.py:117-131 (pykitti): `key: v v v` lines -> {key: float64 array}; lines that hold no numbers are skipped"""
    data = {}
    with open(path) as f:
        for line in f.readlines():
            key, value = line.split(':', 1)
            try:
                data[key] = np.array([float(x) for x in value.split()])
            except ValueError:
                pass
    return data


class KittiRaw(object):
    """kitti_raw_loader.py's KittiRawLoader.  test_scenes: a file or a list of drive names without `_sync` (the reference reads the
    list beside its script; it is reference data, so here the caller passes it); a drive is left out when `name[:-5]` is in it.
    static_frames: None -> frames are chosen by the cumulative-speed rule (oxts fields 8:11, a frame is kept when the norm of the
    speed summed since the last kept frame exceeds min_speed); a file of `date drive frame` lines -> every frame not listed is kept.
    A scene is one camera (02, 03) of one drive, `rel_path` = drive + '_' + camera."""
    cam_ids = ('02', '03')
    date_list = ('2011_09_26', '2011_09_28', '2011_09_29', '2011_09_30', '2011_10_03')

    def __init__(self, dataset_dir, test_scenes, static_frames=None, height=128, width=416, min_speed=2, get_gt=False):
        self.dataset_dir = str(dataset_dir)
        self.height, self.width, self.keep_rows = int(height), int(width), int(height)
        self.min_speed, self.get_gt = min_speed, bool(get_gt)
        self.from_speed = static_frames is None
        self.static_frames = {}
        if static_frames is not None:
            for fr in _lines(static_frames):                             # :35-46
                if not fr.strip():
                    continue
                _, drive, frame_id = fr.split(' ')
                self.static_frames.setdefault(drive, []).append('%.10d' % int(frame_id))
        self.test_scenes = [t for t in _lines(test_scenes) if t]
        self.scenes = [dr for date in self.date_list for dr in _dirs(os.path.join(self.dataset_dir, date))
                       if os.path.basename(dr)[:-5] not in self.test_scenes]          # :48-54

    def _png(self, drive, cid, frame_id):
        return os.path.join(drive, 'image_' + cid, 'data', frame_id + '.png')

    def collect_scenes(self, drive):
        """:56-73 -> one record per camera; [] (for BOTH cameras) when a camera's first frame is missing"""
        name = os.path.basename(drive)
        out = []
        for c in self.cam_ids:
            oxts = _files(os.path.join(drive, 'oxts', 'data'), '*.txt')
            speed = [np.genfromtxt(f)[8:11] for f in oxts]
            frame_id = ['{:010d}'.format(n) for n in range(len(oxts))]
            first = self._png(drive, c, frame_id[0])
            if not os.path.isfile(first):
                return []
            H, W = image_size(first)
            zoom_y, zoom_x = self.height / H, self.width / W             # :112-113: the zoom of frame 0 serves the whole scene
            calib = read_raw_calib_file(os.path.join(os.path.dirname(drive), 'calib_cam_to_cam.txt'))
            P_rect = np.reshape(calib['P_rect_' + c], (3, 4))
            P_rect[0] *= zoom_x
            P_rect[1] *= zoom_y
            scene = {'cid': c, 'dir': drive, 'speed': speed, 'frame_id': frame_id, 'rel_path': name + '_' + c, 'P_rect': P_rect,
                     'intrinsics': P_rect[:, :3]}
            scene['frames'] = self._select(scene)
            out.append(scene)
        return out

    def _select(self, scene):
        """:75-95 -> [(frame id, PNG path)] of the frames the scene keeps"""
        keep = []
        if self.from_speed:
            cum_speed = np.zeros(3)
            for i, speed in enumerate(scene['speed']):
                cum_speed += speed
                if np.linalg.norm(cum_speed) > self.min_speed:
                    keep.append(scene['frame_id'][i])
                    cum_speed *= 0
        else:
            listed = self.static_frames.get(os.path.basename(scene['dir']))
            keep = [f for f in scene['frame_id'] if listed is None or f not in listed]
        return [(f, self._png(scene['dir'], scene['cid'], f)) for f in keep]

    def depth_inputs(self, scene, frame_id):
        """:133-157 -> (raw velodyne points fp32 [N,4], P_velo2im fp64 [3,4] = P_rect_scaled . R_cam2rect . velo2cam)"""
        calib_dir = os.path.dirname(scene['dir'])
        if 'P_velo2im' not in scene:
            cam2cam = read_raw_calib_file(os.path.join(calib_dir, 'calib_cam_to_cam.txt'))
            velo2cam = read_raw_calib_file(os.path.join(calib_dir, 'calib_velo_to_cam.txt'))
            velo2cam = np.hstack((velo2cam['R'].reshape(3, 3), velo2cam['T'][..., np.newaxis]))
            velo2cam = np.vstack((velo2cam, np.array([0, 0, 0, 1.0])))
            R_cam2rect = np.eye(4)
            R_cam2rect[:3, :3] = cam2cam['R_rect_00'].reshape(3, 3)
            scene['P_velo2im'] = np.dot(np.dot(scene['P_rect'], R_cam2rect), velo2cam)
        points = np.fromfile(os.path.join(scene['dir'], 'velodyne_points', 'data', frame_id + '.bin'), dtype=np.float32).reshape(-1, 4)
        return points, scene['P_velo2im']


class Cityscapes(object):
    """cityscapes_loader.py.  A scene is one half (`_0`: frames 0, 2, 4 .. / `_1`: frames 1, 3, 5 ..) of one run of consecutive
    frame numbers of one sequence; frames are chosen by the speed rule AS WRITTEN there: the scalar speed is added to a 3-vector,
    so the norm compared with min_speed = 2 is sqrt(3) times the summed speed.  The bottom quarter (the car's bonnet) is cut:
    int(height * 0.75) rows are kept."""
    get_gt = False

    def __init__(self, dataset_dir, split='train', height=171, width=416):
        self.dataset_dir, self.split = str(dataset_dir), split
        self.height, self.width, self.keep_rows = int(height), int(width), int(int(height) * 0.75)
        self.min_speed = 2
        self.scenes = _dirs(os.path.join(self.dataset_dir, 'leftImg8bit_sequence', split))

    def _png(self, city, scene_id, frame_id):
        return os.path.join(city, '{}_{}_{}_leftImg8bit.png'.format(os.path.basename(city), scene_id, frame_id))

    def collect_scenes(self, city):
        """:26-65"""
        name = os.path.basename(city)
        scenes = {}
        for f in _files(city, '*.png'):
            scene_id, frame_id = os.path.basename(f).split('_')[1:3]
            scenes.setdefault(scene_id, []).append(frame_id)
        out = []
        for scene_id, ids in scenes.items():
            runs, previous = [], None
            for i in ids:                                               # connex sub-sequences
                if previous is None or int(i) - int(previous) > 1:
                    runs.append([])
                runs[-1].append(i)
                previous = i
            intrinsics = self.load_intrinsics(city, scene_id)
            for run in runs:
                speeds = [self.load_speed(city, scene_id, i) for i in run]
                for half in (0, 1):
                    scene = {'city': city, 'scene_id': scene_id, 'rel_path': '%s_%s_%s_%d' % (name, scene_id, run[0], half),
                             'intrinsics': intrinsics, 'frame_ids': run[half::2], 'speeds': speeds[half::2]}
                    scene['frames'] = self._select(scene)
                    out.append(scene)
        return out

    def load_intrinsics(self, city, scene_id):
        """:67-91: the camera JSON's intrinsics times the zoom of the frame that JSON is named after"""
        name = os.path.basename(city)
        camera_file = _files(os.path.join(self.dataset_dir, 'camera', self.split, name), '{}_{}_*_camera.json'.format(name, scene_id))[0]
        frame_id = os.path.basename(camera_file).split('_')[2]
        with open(camera_file) as f:
            camera = json.load(f)
        k = camera['intrinsic']
        intrinsics = np.array([[k['fx'], 0, k['u0']], [0, k['fy'], k['v0']], [0, 0, 1]])
        H, W = image_size(self._png(city, scene_id, frame_id))
        intrinsics[0] *= self.width / W
        intrinsics[1] *= self.height / H
        return intrinsics

    def load_speed(self, city, scene_id, frame_id):
        name = os.path.basename(city)
        with open(os.path.join(self.dataset_dir, 'vehicle_sequence', self.split, name,
                               '{}_{}_{}_vehicle.json'.format(name, scene_id, frame_id))) as f:
            return json.load(f)['speed']

    def _select(self, scene):
        """:101-109"""
        keep = []
        cum_speed = np.zeros(3)
        for i, frame_id in enumerate(scene['frame_ids']):
            cum_speed += scene['speeds'][i]
            if np.linalg.norm(cum_speed) > self.min_speed:
                keep.append((frame_id, self._png(scene['city'], scene['scene_id'], frame_id)))
                cum_speed *= 0
        return keep


# ------------------------------------------------------------------------------------------------------------ the device side
_tables = {}


def _axis_table(in_size, out_size, device):
    """resample_table as the kernel reads it: int32 [out * (1 + taps)] = first[out], weights[out][taps]; cached per device"""
    key = (int(in_size), int(out_size), str(device))
    if key not in _tables:
        first, q = resample_table(in_size, out_size)
        _tables[key] = (torch.from_numpy(np.concatenate([first.reshape(-1), q.reshape(-1)]).astype(np.int32)).to(device), int(q.shape[1]))
    return _tables[key]


def resize_u8(src, h, w, h_keep=None):
    """uint8 [N,H,W,3] on the device -> uint8 [N,h_keep,w,3]: rows 0 .. h_keep-1 of Image.resize((w, h), BILINEAR), bit for bit"""
    if src.dtype != torch.uint8 or src.dim() != 4 or src.shape[3] != 3:
        raise ValueError("resize_u8: frames must be uint8 [N,H,W,3], got %s %s" % (src.dtype, tuple(src.shape)))
    h_keep = h if h_keep is None else h_keep
    N, H, W = (int(v) for v in src.shape[:3])
    E, dev = engine(), src.device
    htab, KH = _axis_table(W, w, dev)
    vtab, KV = _axis_table(H, h, dev)
    dst = torch.empty((N, h_keep, w, 3), dtype=torch.uint8, device=dev)
    ws = torch.empty(max(1, int(E.call("cc_frames_resize_u8_ws", N, H, w))), dtype=torch.uint8, device=dev)
    E.call("cc_frames_resize_u8", src.contiguous(), dst, htab, KH, vtab, KV, ws, N, H, W, h, w, h_keep, STREAM)
    return dst


class _Clock(object):
    def __init__(self, cuda):
        self.cuda, self.seconds = cuda, {k: 0.0 for k in STAGES}

    def add(self, stage, t0, sync=False):
        if sync and self.cuda:
            torch.cuda.current_stream().synchronize()
        t1 = time.perf_counter()
        self.seconds[stage] += t1 - t0
        return t1


def split_draws(folders):
    """prepare_train_data.py:78-89 on `folders` in the order given: one draw per folder from RandomState(8964) (np.random.seed(8964)
    + np.random.random() there; the global generator stays untouched here) -> (train, val)"""
    rng = np.random.RandomState(SPLIT_SEED)
    train, val = [], []
    for name in folders:
        (val if rng.random_sample() < 0.1 else train).append(name)
    return train, val


def _jpgs(folder):
    return [n for n in (os.listdir(folder) if os.path.isdir(folder) else []) if fnmatch.fnmatchcase(n, '*.jpg')]


def prepare(loader, dump_root, store_cache=None, sequence_length=5, device='cuda', workers=4, chunk_frames=64, keep_frames=False,
            max_bytes=None):
    """-> {'scenes': [rel_path ..] (the folders that stay), 'frames': {rel_path: [frame id ..]}, 'train': [..], 'val': [..],
    'seconds': {stage: s}, 'stores': {name: samples}}; with keep_frames (tests) also 'kept': {rel_path: uint8 [n,rows,w,3]}, the
    resized frames, and 'kept_ids': {rel_path: [frame id ..]}, both including the scenes removed for fewer than three frames.
    max_bytes: refuse (ValueError, before anything is allocated) when the resized frames that stay resident for the stores
    (store_cache) need more device memory than this."""
    dump_root = str(dump_root)
    device = torch.device(device)
    cuda = device.type == "cuda"
    clock = _Clock(cuda)
    h, w, rows = loader.height, loader.width, loader.keep_rows
    get_gt = loader.get_gt
    chunk_frames = max(1, int(chunk_frames))
    if store_cache is not None and os.path.dirname(os.path.abspath(store_cache)) == os.path.abspath(dump_root):
        raise ValueError("store_cache %s lies inside dump_root: the split would list it as a scene" % store_cache)
    os.makedirs(dump_root, exist_ok=True)

    with ThreadPoolExecutor(max_workers=max(1, int(workers))) as pool:
        # ---- the plan: scenes, frames, and -- since the frame choice reads no pixel -- the split, before the first decode
        t = time.perf_counter()
        scenes = [s for group in pool.map(loader.collect_scenes, loader.scenes) for s in group]
        stay = set(os.path.basename(d) for d in _dirs(dump_root))
        for s in scenes:
            folder = os.path.join(dump_root, s['rel_path'])
            if len(set(_jpgs(folder)) | set(f + '.jpg' for f, _ in s['frames'])) >= 3:
                stay.add(s['rel_path'])
            else:
                stay.discard(s['rel_path'])
        plan_train, plan_val = split_draws(sorted(stay))
        resident = store_cache is not None
        if resident and max_bytes is not None:
            F = sum(len(s['frames']) for s in scenes if s['rel_path'] in stay)
            need = F * rows * w * 3 + 8 * F + (4 * h * w * sum(len(s['frames']) for s in scenes if s['rel_path'] in plan_val) if get_gt else 0)
            if need > max_bytes:
                raise ValueError("%s: %d frames of %d x %d need %d bytes, more than max_bytes = %d" % (dump_root, F, rows, w, need, max_bytes))
        t = clock.add("crawl", t)

        staging = {}                                                    # (H, W) -> pinned [chunk,H,W,3]; one per source size
        back = torch.empty((chunk_frames, rows, w, 3), dtype=torch.uint8, pin_memory=cuda)
        held, held_depth, kept, kept_ids, frames_of = {}, {}, {}, {}, {}

        def decode(job):
            path, out = job
            a = load_png_rgb8(path)
            if a.shape != out.shape:
                raise ValueError("%s: %d x %d, the scene's frames are %d x %d" % (path, a.shape[0], a.shape[1], out.shape[0], out.shape[1]))
            out[...] = a

        def encode(job):
            from PIL import Image
            path, a = job
            Image.fromarray(a).save(path)                               # scipy.misc.imsave: toimage(arr).save(name), default quality

        for s in scenes:
            folder = os.path.join(dump_root, s['rel_path'])
            os.makedirs(folder, exist_ok=True)
            K = s['intrinsics']
            with open(os.path.join(folder, 'cam.txt'), 'w') as f:
                f.write(CAM_FORMAT % (K[0, 0], K[0, 2], K[1, 1], K[1, 2]))
            names = s['frames']
            keep_dev = (resident and s['rel_path'] in stay) or keep_frames
            want_depth = get_gt and s['rel_path'] in plan_val          # a train scene's maps are deleted by the split: not made
            parts, dparts = [], []
            for lo in range(0, len(names), chunk_frames):
                part = names[lo:lo + chunk_frames]
                n = len(part)
                H, W = image_size(part[0][1])
                if (H, W) not in staging:
                    staging[(H, W)] = torch.empty((chunk_frames, H, W, 3), dtype=torch.uint8, pin_memory=cuda)
                buf = staging[(H, W)]
                t = time.perf_counter()
                list(pool.map(decode, [(p, buf.numpy()[i]) for i, (_, p) in enumerate(part)]))
                t = clock.add("decode", t)
                src = buf[:n].to(device, non_blocking=True) if cuda else buf[:n]
                t = clock.add("upload", t, sync=True)
                out = resize_u8(src, h, w, rows)
                t = clock.add("resize", t, sync=True)
                if want_depth:
                    for fid, _ in part:
                        pts, P = loader.depth_inputs(s, fid)
                        dparts.append(velo_depth(torch.from_numpy(pts).to(device), torch.from_numpy(np.ascontiguousarray(P)).to(device), h, w))
                    t = clock.add("depth", t, sync=True)
                back[:n].copy_(out, non_blocking=True)
                host_depth = [d.cpu().numpy() for d in dparts[-n:]] if want_depth else []
                t = clock.add("download", t, sync=True)
                list(pool.map(encode, [(os.path.join(folder, fid + '.jpg'), back.numpy()[i]) for i, (fid, _) in enumerate(part)]))
                for (fid, _), d in zip(part, host_depth):
                    np.save(os.path.join(folder, fid + '.npy'), d)
                t = clock.add("encode", t)
                if keep_dev:
                    parts.append(out)
            if keep_dev and parts:
                held[s['rel_path']] = torch.cat(parts) if len(parts) > 1 else parts[0]
                if keep_frames:                                          # (also of a scene that is removed next)
                    kept[s['rel_path']] = held[s['rel_path']].cpu().numpy()
                    kept_ids[s['rel_path']] = [fid for fid, _ in names]
            if len(_jpgs(folder)) < 3:                                   # prepare_train_data.py:50-51
                shutil.rmtree(folder)
                held.pop(s['rel_path'], None)
                continue
            frames_of[s['rel_path']] = [fid for fid, _ in names]
            if dparts:
                held_depth[s['rel_path']] = torch.stack(dparts)

    # ---- the split, prepare_train_data.py:78-89, on the folders as they are now
    t = time.perf_counter()
    folders = [os.path.basename(d) for d in _dirs(dump_root)]
    train, val = split_draws(folders)
    if (train, val) != (plan_train, plan_val):
        raise RuntimeError("%s: its scene folders changed while they were written (planned %d train / %d val, found %d / %d)"
                           % (dump_root, len(plan_train), len(plan_val), len(train), len(val)))
    with open(os.path.join(dump_root, 'train.txt'), 'w') as tf:
        for name in train:
            tf.write('{}\n'.format(name))
            for gt_file in _files(os.path.join(dump_root, name), '*.npy'):
                os.remove(gt_file)
    with open(os.path.join(dump_root, 'val.txt'), 'w') as vf:
        for name in val:
            vf.write('{}\n'.format(name))
    t = clock.add("split", t)

    stores = {}
    if resident:
        stores = _write_stores(dump_root, store_cache, sequence_length, device, held, held_depth, frames_of, get_gt)
        clock.add("stores", t, sync=True)
    record = {'scenes': sorted(frames_of), 'frames': frames_of, 'train': train, 'val': val, 'seconds': clock.seconds, 'stores': stores}
    if keep_frames:
        record['kept'], record['kept_ids'] = kept, kept_ids
    return record


def _frame_of(dump_root, held, frames_of, path):
    """the resized frame (with held = the depth maps: the map) of the frame that was written to `path`, a device view"""
    scene, name = os.path.relpath(path, dump_root).replace(os.sep, "/").split("/")
    ids = frames_of.get(scene, [])
    if scene not in held or name[:-4] not in ids:
        raise ValueError("%s: a frame this run did not write; stores can only be made of a dump this run wrote whole" % path)
    return held[scene][ids.index(name[:-4])]


def _write_stores(dump_root, store_cache, sequence_length, device, held, held_depth, frames_of, get_gt):
    """DIR/train, DIR/val_unsup (FrameStore) and, with get_gt, DIR/val_depth (DepthValStore) from the frames on the device: the
    tables are those `FrameStore.build` / `DepthValStore.build` derive from the folders just written (the same crawl, cam.txt
    parsed back from its text), the frames are the resized ones, never JPEG-coded.  A set without a sample is not written."""
    E = engine()
    done = {}
    for name, is_train in (("train", True), ("val_unsup", False)):
        scenes, intrinsics, found = crawl(dump_root, is_train, sequence_length)
        if not found:
            done[name] = 0
            continue
        paths, samples, sample_scene = frame_tables(found)
        frames = torch.stack([_frame_of(dump_root, held, frames_of, p) for p in paths])
        minmax = torch.empty((len(paths), 2), dtype=torch.float32, device=device)
        E.call("cc_store_minmax", frames, minmax, len(paths), int(np.prod(frames.shape[1:])), STREAM)
        FrameStore(frames, minmax, intrinsics, samples, sample_scene, scenes).save(os.path.join(store_cache, name))
        done[name] = len(found)
    if get_gt:
        _, imgs, depths = crawl_validation(dump_root)
        if imgs:
            frames = torch.stack([_frame_of(dump_root, held, frames_of, p) for p in imgs])
            depth = torch.stack([_frame_of(dump_root, held_depth, frames_of, p) for p in imgs])
            names = [os.path.relpath(p, dump_root).replace(os.sep, "/") for p in imgs]
            DepthValStore(frames, depth, names).save(os.path.join(store_cache, "val_depth"))
        done["val_depth"] = len(imgs)
    return done
