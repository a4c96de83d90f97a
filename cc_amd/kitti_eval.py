"""KITTI evaluation on the device: Eigen-split depth (reference test_disp.py with kitti_eval/depth_evaluation_utils.py),
odometry ATE / RE (test_pose.py with kitti_eval/pose_evaluation_utils.py), KITTI 2015 optical flow (test_flow.py) and motion
segmentation (test_mask.py), the last two on datasets/validation_flow.py's tree.

Thin wrappers over the HIP entries of cc_amd/csrc/kitti_eval.hip and kitti_flow_eval.hip (include/ccengine.h, "KITTI
evaluation" and "KITTI 2015 flow and mask evaluation"), the four evaluation loops, dataset readers that mirror the reference's
metadata code on `pathlib` and PIL, and a command line:

    python -m cc_amd.kitti_eval depth --pretrained-dispnet D.pth.tar [--pretrained-posenet P.pth.tar] --dataset-dir RAW \\
        --dataset-list test_files_eigen.txt
    python -m cc_amd.kitti_eval pose P.pth.tar --dataset-dir ODOMETRY --sequences 09 10
    python -m cc_amd.kitti_eval flow --kitti-dir KITTI2015 --pretrained-disp D --pretrained-pose P --pretrained-mask M \\
        --pretrained-flow F
    python -m cc_amd.kitti_eval mask --kitti-dir KITTI2015 --pretrained-disp D --pretrained-pose P --pretrained-mask M \\
        --pretrained-flow F

The ground-truth depth map, the spline zoom of the prediction, the masked median scaling and the errors all run as kernels; the
evaluation loops read results back to the host once, after the loop.  Readers return what the files hold (uint8 frames, raw
velodyne points, P_velo2im, displacements, ground-truth poses); no depth map is built on the host.
"""
import argparse
import datetime
import math
import pathlib
import struct
import types
import zlib

import numpy as np
import torch

from ._lib import engine, STREAM

ERROR_NAMES = ['abs_rel', 'sq_rel', 'rms', 'log_rms', 'a1', 'a2', 'a3']       # test_disp.py:144
POSE_ERROR_NAMES = ['ATE', 'RE']                                               # test_pose.py:96
ROTATION_MODES = {'euler': 0, 'quat': 1}
FLOW_ERROR_NAMES = ['epe_total', 'epe_sp', 'epe_mv', 'Fl', 'epe_total_gt_mask', 'epe_sp_gt_mask', 'epe_mv_gt_mask',
                    'Fl_gt_mask']                                              # test_flow.py:106
MASK_COUNT_NAMES = ['tp_0', 'fp_0', 'fn_0', 'tp_1', 'fp_1', 'fn_1']            # test_mask.py:105
MASK_ROWS = ('full', 'census', 'bare')                                         # the rows of the counts buffer
NORM_FIELDS = ("rigidity_mask", "rigidity_mask_census", "rigidity_mask_combined", "flow_fwd_non_rigid", "flow_fwd_rigid",
               "total_flow")
PNG_SIGNATURE = b'\x89PNG\r\n\x1a\n'


def _ws(nbytes, dev):
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev)


# ------------------------------------------------------------------------------------------------------------ kernel wrappers
def velo_depth(points, P_velo2im, H, W):
    """generate_depth_map (depth_evaluation_utils.py:148-191): raw velodyne points [N,4] fp32 and P_velo2im [3,4] fp64, both
    on the device -> sparse ground-truth depth [H,W] fp32 (the reference's fp64 map, cast)."""
    assert points.dim() == 2 and points.shape[1] == 4 and points.dtype == torch.float32, "velo_depth: points must be fp32 [N,4]"
    assert P_velo2im.shape == (3, 4) and P_velo2im.dtype == torch.float64, "velo_depth: P_velo2im must be fp64 [3,4]"
    dev = points.device
    e = engine()
    depth = torch.empty((H, W), dtype=torch.float32, device=dev)
    e.call("cc_velo_depth", points.contiguous(), points.shape[0], P_velo2im.contiguous(), depth, H, W,
           _ws(e.call("cc_velo_depth_ws", H, W), dev), STREAM)
    return depth


def spline_zoom(src, H, W, lo, hi):
    """scipy.ndimage.zoom(src, (H/h, W/w)) (order 3, mode 'constant') then .clip(lo, hi), test_disp.py:125; bit-exact with
    SciPy.  src [h,w] or [B,h,w] fp32 -> [H,W] or [B,H,W] fp32."""
    squeeze = src.dim() == 2
    s = src.detach().float().contiguous()
    if squeeze:
        s = s.unsqueeze(0)
    B, h, w = s.shape
    e = engine()
    dst = torch.empty((B, H, W), dtype=torch.float32, device=s.device)
    e.call("cc_spline_zoom", s, B, h, w, dst, H, W, float(np.float32(lo)), float(np.float32(hi)),
           _ws(e.call("cc_spline_zoom_ws", B, h, w), s.device), STREAM)
    return dst[0] if squeeze else dst


def eigen_errors(gt, pred, min_depth=1e-3, max_depth=80, displacements=None, pose_norm=None, out=None):
    """One image of test_disp.py:124-141: gt, pred [H,W] fp32 (pred already zoomed and clipped) -> [2,7] fp64 device tensor of
    compute_errors (ERROR_NAMES) inside generate_mask.  Row 1: median scaling (np.median, the mean of the middle pair for an even
    count).  Row 0: the PoseNet scale from displacements [R] (fp64) and the norms [R] of the pose network's translations, zeros
    without them.  out: an optional [2,7] fp64 device tensor (e.g. a row of a per-image buffer) to write into."""
    assert gt.dim() == 2 and pred.shape == gt.shape, "eigen_errors: gt and pred must be [H,W] of one shape"
    assert (displacements is None) == (pose_norm is None), "eigen_errors: displacements and pose_norm go together"
    H, W = gt.shape
    dev = gt.device
    if out is None:
        out = torch.empty((2, 7), dtype=torch.float64, device=dev)
    assert out.shape == (2, 7) and out.dtype == torch.float64 and out.is_contiguous()
    R = 0
    if displacements is not None:
        displacements = displacements.to(dev, torch.float64).contiguous()
        pose_norm = pose_norm.detach().float().contiguous()
        R = displacements.numel()
        assert pose_norm.numel() == R, "eigen_errors: one pose norm per displacement"
    e = engine()
    e.call("cc_eigen_errors", gt.float().contiguous(), pred.float().contiguous(), H, W, float(min_depth), float(max_depth),
           displacements, pose_norm, R, out, _ws(e.call("cc_eigen_errors_ws", H, W), dev), STREAM)
    return out


def pose_snippet_errors(pred, gt_seq, first, rotation_mode='euler', step=1, want_final=False):
    """test_pose.py:69-91 + compute_pose_error for every snippet of one sequence: pred [S,L-1,6] network poses, gt_seq [F,3,4]
    fp64 raw sequence poses, first [S] int32 first frame of each snippet (frames first + i*step) -> err [S,2] fp64 (ATE, RE)
    (and the composed poses [S,L,3,4] fp64 with want_final)."""
    assert pred.dim() == 3 and pred.shape[2] == 6, "pose_snippet_errors: pred must be [S,L-1,6]"
    S, L = pred.shape[0], pred.shape[1] + 1
    dev = pred.device
    assert gt_seq.dim() == 3 and gt_seq.shape[1:] == (3, 4), "pose_snippet_errors: gt_seq must be [F,3,4]"
    first = first.to(dev, torch.int32).contiguous()
    assert first.numel() == S
    err = torch.empty((S, 2), dtype=torch.float64, device=dev)
    final = torch.empty((S, L, 3, 4), dtype=torch.float64, device=dev) if want_final else None
    engine().call("cc_pose_snippet_errors", pred.detach().float().contiguous(), gt_seq.to(dev, torch.float64).contiguous(), first, S,
                  L, gt_seq.shape[0], int(step), ROTATION_MODES[rotation_mode], err, final, STREAM)
    return (err, final) if want_final else err


def png16_scanlines(data):
    """The inflated scanlines of a non-interlaced 16-bit RGB PNG held in `data` (bytes): IHDR parsed, the IDAT chunks
    concatenated and inflated with zlib, the stream split into -> (ftype [H] uint8 the filter byte of every row, rows
    [H, stride] uint8 its 6*W filtered bytes padded with zeros to a multiple of 8, W).  ValueError for anything that is not
    bit depth 16, colour type 2, interlace 0."""
    if data[:8] != PNG_SIGNATURE:
        raise ValueError("not a PNG file")
    pos, idat, ihdr = 8, [], None
    while pos + 8 <= len(data):
        length, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + length]
        pos += 12 + length
        if kind == b'IHDR':
            ihdr = struct.unpack(">IIBBBBB", body)
        elif kind == b'IDAT':
            idat.append(body)
        elif kind == b'IEND':
            break
    if ihdr is None:
        raise ValueError("PNG without an IHDR chunk")
    W, H, depth, colour, _, _, interlace = ihdr
    if (depth, colour, interlace) != (16, 2, 0):
        raise ValueError("flow PNG must be 16-bit RGB, not interlaced (bit depth %d, colour type %d, interlace %d)"
                         % (depth, colour, interlace))
    raw = np.frombuffer(zlib.decompress(b''.join(idat)), dtype=np.uint8)
    if raw.size != H * (1 + 6 * W):
        raise ValueError("PNG data holds %d bytes, %d x %d 16-bit RGB needs %d" % (raw.size, W, H, H * (1 + 6 * W)))
    raw = raw.reshape(H, 1 + 6 * W)
    ftype = raw[:, 0].copy()
    if ftype.size and ftype.max() > 4:
        raise ValueError("PNG filter type %d" % int(ftype.max()))
    rows = np.zeros((H, (6 * W + 7) // 8 * 8), dtype=np.uint8)
    rows[:, :6 * W] = raw[:, 1:]
    return ftype, rows, W


def png16_flow_decode(ftype, rows, W):
    """cc_png16_flow_decode: ftype [N,H] and rows [N,H,stride] uint8 on the device (png16_scanlines of N files of one size)
    -> [N,3,H,W] fp32 = u, v, valid of flow_read_png (flowutils/flow_io.py:96-117)."""
    assert ftype.dim() == 2 and rows.dim() == 3 and rows.shape[:2] == ftype.shape, "png16_flow_decode: ftype [N,H], rows [N,H,stride]"
    assert ftype.dtype == torch.uint8 and rows.dtype == torch.uint8
    N, H, stride = rows.shape
    gt = torch.empty((N, 3, H, W), dtype=torch.float32, device=rows.device)
    engine().call("cc_png16_flow_decode", ftype.contiguous(), rows.contiguous(), N, H, int(W), stride, gt, STREAM)
    return gt


def read_flow_png(path, device='cuda'):
    """flow_read_png + torch.FloatTensor(np.dstack((u, v, valid)).transpose(2, 0, 1)) (validation_flow.py:125-128) of a KITTI
    flow ground-truth file -> [3,H,W] fp32 on the device.  The host inflates; the PNG filters are undone by the kernel."""
    with open(str(path), 'rb') as f:
        ftype, rows, W = png16_scanlines(f.read())
    dev = torch.device(device)
    return png16_flow_decode(torch.from_numpy(ftype).to(dev)[None], torch.from_numpy(rows).to(dev)[None], W)[0]


def rigidity_composition_norm(explainability_mask, flow_cam, flow_fwd, THRESH, want=NORM_FIELDS):
    """test_mask.py:129-138 per sample (the reference runs batch size 1, where its .max() over the batch is the sample's):
    explainability_mask [B,MC>=3,H,W], flow_cam / flow_fwd [B,2,H,W] -> namespace with rigidity_mask (the bare MaskNet mask),
    rigidity_mask_census, rigidity_mask_combined [B,1,H,W] (0/1 fp32, bit-exact with torch) and flow_fwd_non_rigid,
    flow_fwd_rigid, total_flow [B,2,H,W].  `want`: the fields to produce (the others are None)."""
    B, MC, H, W = explainability_mask.shape
    assert flow_cam.shape == (B, 2, H, W) and flow_fwd.shape == (B, 2, H, W), "rigidity_composition_norm: flows must be [B,2,H,W] of the mask"
    unknown = set(want) - set(NORM_FIELDS)
    assert not unknown, "rigidity_composition_norm: unknown fields %s" % sorted(unknown)
    m = explainability_mask.detach().float().contiguous()
    fc, ff = flow_cam.detach().float().contiguous(), flow_fwd.detach().float().contiguous()
    o = {k: (torch.empty((B, 1 if k.startswith("rigidity") else 2, H, W), dtype=torch.float32, device=m.device) if k in want else None)
         for k in NORM_FIELDS}
    e = engine()
    e.call("cc_rigidity_compose_norm", m, MC, fc, ff, o["rigidity_mask"], o["rigidity_mask_census"], o["rigidity_mask_combined"],
           o["flow_fwd_non_rigid"], o["flow_fwd_rigid"], o["total_flow"], float(THRESH), B, H, W,
           _ws(e.call("cc_rigidity_compose_norm_ws", B), m.device), STREAM)
    return types.SimpleNamespace(**o)


def mask_iou_counts(obj_map, semantic, masks, counts=None):
    """mask_error (test_mask.py:224-262) of up to three predicted masks [h,w] fp32 (None: skipped) against obj_map / semantic
    [Hg,Wg] uint8, all on the device: ADDS tp_0, fp_0, fn_0, tp_1, fp_1, fn_1 of mask k into row k of counts ([3,6] int64 on the
    device; a zeroed one is made when None) -> counts."""
    masks = list(masks) + [None] * (3 - len(masks))
    assert len(masks) == 3, "mask_iou_counts: at most three masks"
    assert obj_map.dim() == 2 and semantic.shape == obj_map.shape, "mask_iou_counts: obj_map and semantic must be [Hg,Wg] of one shape"
    assert obj_map.dtype == torch.uint8 and semantic.dtype == torch.uint8, "mask_iou_counts: the maps are uint8"
    hw = {tuple(m.shape) for m in masks if m is not None}
    assert len(hw) == 1 and len(next(iter(hw))) == 2, "mask_iou_counts: masks must be [h,w] of one shape"
    h, w = next(iter(hw))
    if counts is None:
        counts = torch.zeros((3, 6), dtype=torch.int64, device=obj_map.device)
    assert counts.shape == (3, 6) and counts.dtype == torch.int64 and counts.is_contiguous()
    pm = [None if m is None else m.detach().float().contiguous() for m in masks]
    engine().call("cc_mask_iou_counts", obj_map.contiguous(), semantic.contiguous(), obj_map.shape[0], obj_map.shape[1], pm[0],
                  pm[1], pm[2], h, w, counts, STREAM)
    return counts


def mask_ious(counts):
    """test_mask.py:199-209 for the summed counts [3,6] -> {'full' | 'census' | 'bare': (iou, bg_iou, fg_iou)} in fp64"""
    c = np.asarray(counts, dtype=np.float64).reshape(3, 6)
    out = {}
    with np.errstate(divide='ignore', invalid='ignore'):
        for k, name in enumerate(MASK_ROWS):
            bg = c[k, 0] / (c[k, 0] + c[k, 1] + c[k, 2])
            fg = c[k, 3] / (c[k, 3] + c[k, 4] + c[k, 5])
            out[name] = ((bg + fg) / 2, bg, fg)
    return out


# ------------------------------------------------------------------------------------------------------------------- readers
def read_text_lines(file_path):
    with open(file_path, 'r') as f:
        return [l.rstrip() for l in f.readlines()]


def read_calib_file(path):
    """depth_evaluation_utils.py:116-133: `key: values` lines; values made only of float characters become float arrays."""
    float_chars = set("0123456789.e+- ")
    data = {}
    with open(path, 'r') as f:
        for line in f.readlines():
            key, value = line.split(':', 1)
            value = value.strip()
            data[key] = value
            if float_chars.issuperset(value):
                try:
                    data[key] = np.array(list(map(float, value.split(' '))))
                except ValueError:
                    pass
    return data


def velo_to_image(calib_dir, cam=2):
    """P_velo2im [3,4] fp64 = P_rect . R_cam2rect . velo2cam from calib_cam_to_cam.txt / calib_velo_to_cam.txt
    (depth_evaluation_utils.py:150-160)."""
    calib_dir = pathlib.Path(calib_dir)
    cam2cam = read_calib_file(calib_dir / 'calib_cam_to_cam.txt')
    velo2cam = read_calib_file(calib_dir / 'calib_velo_to_cam.txt')
    velo2cam = np.hstack((velo2cam['R'].reshape(3, 3), velo2cam['T'][..., np.newaxis]))
    velo2cam = np.vstack((velo2cam, np.array([0, 0, 0, 1.0])))
    R_cam2rect = np.eye(4)
    R_cam2rect[:3, :3] = cam2cam['R_rect_00'].reshape(3, 3)
    P_rect = cam2cam['P_rect_0' + str(cam)].reshape(3, 4)
    return np.dot(np.dot(P_rect, R_cam2rect), velo2cam)


def load_velodyne_points(file_name):
    """the raw [N,4] fp32 points of a velodyne .bin (the kernel ignores the fourth value, which the reference sets to 1)"""
    return np.fromfile(str(file_name), dtype=np.float32).reshape(-1, 4)


def imread(path):
    """scipy.misc.imread of an RGB image -> uint8 [H,W,3]"""
    from PIL import Image
    with Image.open(str(path)) as im:
        if im.mode != 'RGB':
            im = im.convert('RGB')
        return np.asarray(im, dtype=np.uint8).copy()


def get_displacements(oxts_root, index, shifts):
    """depth_evaluation_utils.py:58-65: oxts speed (|v| of fields 8:11) x |delta t| to each reference frame."""
    oxts_root = pathlib.Path(oxts_root)
    with open(oxts_root / 'timestamps.txt') as f:
        timestamps = [datetime.datetime.strptime(ts[:-3], "%Y-%m-%d %H:%M:%S.%f").timestamp() for ts in f.read().splitlines()]
    oxts_data = np.genfromtxt(oxts_root / 'data' / '{:010d}.txt'.format(index))
    speed = np.linalg.norm(oxts_data[8:11])
    assert all(0 <= index + shift < len(timestamps) for shift in shifts), str([index + shift for shift in shifts])
    return [speed * abs(timestamps[index] - timestamps[index + shift]) for shift in shifts]


class KittiRawEigen(object):
    """The Eigen test split of KITTI raw (depth_evaluation_utils.py:17-37 and read_scene_data :68-106).  test_files: the list
    of `date/scene/image_0X/data/index.png` paths relative to root.  Item i -> dict of 'tgt' (uint8 [H,W,3]), 'ref' (uint8
    frames at the seq_length - 1 shifts; a missing one is replaced by the target, shift 0), 'path', 'velo' (raw points [N,4]
    fp32), 'P_velo2im' ([3,4] fp64) and 'displacements' (fp64 [seq_length - 1])."""

    def __init__(self, root, test_files, seq_length=3, min_depth=1e-3, max_depth=100, step=1):
        self.root = pathlib.Path(root)
        self.min_depth, self.max_depth = min_depth, max_depth
        self.calib_dirs, self.gt_files, self.img_files, self.displacements, self.cams = [], [], [], [], []
        demi_length = (seq_length - 1) // 2
        shift_range = [step * i for i in list(range(-demi_length, 0)) + list(range(1, demi_length + 1))]
        for sample in test_files:
            tgt_img_path = self.root / sample
            date, scene, cam_id, _, index = sample[:-4].split('/')
            ref_imgs_path = [tgt_img_path.parent / '{:010d}.png'.format(int(index) + shift) for shift in shift_range]
            caped_shift_range = shift_range[:]
            for i, img in enumerate(ref_imgs_path):
                if not img.is_file():
                    ref_imgs_path[i] = tgt_img_path
                    caped_shift_range[i] = 0
            vel_path = self.root / date / scene / 'velodyne_points' / 'data' / '{}.bin'.format(index[:10])
            if tgt_img_path.is_file():
                self.gt_files.append(vel_path)
                self.calib_dirs.append(self.root / date)
                self.img_files.append([tgt_img_path, ref_imgs_path])
                self.cams.append(int(cam_id[-2:]))
                self.displacements.append(get_displacements(self.root / date / scene / 'oxts', int(index), caped_shift_range))
            else:
                print('{} missing'.format(tgt_img_path))

    def __getitem__(self, i):
        return {'tgt': imread(self.img_files[i][0]),
                'ref': [imread(img) for img in self.img_files[i][1]],
                'path': self.img_files[i][0],
                'velo': load_velodyne_points(self.gt_files[i]),
                'P_velo2im': velo_to_image(self.calib_dirs[i], self.cams[i]),
                'displacements': np.array(self.displacements[i], dtype=np.float64)}

    def __len__(self):
        return len(self.img_files)


class KittiOdometry(object):
    """KITTI odometry sequences (pose_evaluation_utils.py:10-34 and read_scene_data :37-62): every directory of
    root/sequences matching one of `sequences` (glob patterns), in sorted order.  self.sequences: per sequence a dict of 'name',
    'img_files' (sorted image_2/*.png), 'poses' ([F,3,4] fp64 from root/poses/<name>.txt) and 'first' (int32 first frame of
    every snippet of seq_length frames at `step`).  len() counts snippets; n_frames counts frames, which is what the reference's
    __len__ returns (see evaluate_pose)."""

    def __init__(self, root, sequences, seq_length=3, step=1):
        self.root = pathlib.Path(root)
        self.seq_length, self.step = seq_length, step
        demi_length = (seq_length - 1) // 2
        dirs = set()
        for seq in sequences:
            dirs |= {d for d in (self.root / 'sequences').glob(seq) if d.is_dir()}
        self.sequences = []
        for d in sorted(dirs):
            poses = np.genfromtxt(self.root / 'poses' / '{}.txt'.format(d.name)).astype(np.float64).reshape(-1, 3, 4)
            imgs = sorted((d / 'image_2').glob('*.png'))
            tgt = np.arange(demi_length, len(imgs) - demi_length)
            self.sequences.append({'name': d.name, 'img_files': imgs, 'poses': poses,
                                   'first': (tgt - demi_length * step).astype(np.int32)})

    @property
    def n_frames(self):
        return sum(len(s['img_files']) for s in self.sequences)

    def __len__(self):
        return sum(len(s['first']) for s in self.sequences)


def read_raw_calib_file(path):
    """validation_flow.py:41-55: `key: values` lines; every value that parses as floats becomes an array, the rest is dropped."""
    data = {}
    with open(str(path), 'r') as f:
        for line in f.readlines():
            key, value = line.split(':', 1)
            try:
                data[key] = np.array([float(x) for x in value.split()])
            except ValueError:
                pass
    return data


def _imread_gray(path):
    from PIL import Image
    with Image.open(str(path)) as im:
        return np.array(im)


class Kitti2015Flow(object):
    """The KITTI 2015 scene-flow tree as ValidationFlow / ValidationMask read it (datasets/validation_flow.py:95-185): target
    frame data_scene_flow_multiview/<phase>/image_2/<index>_10.png, reference frames _08 _09 _11 _12 at sequence_length 5
    (seq_ids), ground truth data_scene_flow/<phase>/<occ>/<index>_10.png, calibration
    data_scene_flow_calib/<phase>/calib_cam_to_cam/<index>.txt, obj_map data_scene_flow/<phase>/obj_map/<index>_10.png and, with
    with_semantic, semantic_labels/<phase>/semantic/<index>_10.png.  Item i -> dict of what the files hold: 'tgt' / 'ref' uint8
    [H,W,3] frames, 'intrinsics' = P_rect_02[:, :3] as float32, 'flow_path' (decoded on the device: read_flow_png), 'obj_map'
    [H,W] as stored (ones where the file is missing, :121-124) and 'semantic' [H,W] or None.  `kitti2015_item` turns an item
    into the reference loader's tuple."""

    def __init__(self, root, sequence_length=5, phase='training', occ='flow_occ', N=200, with_semantic=False):
        self.root = pathlib.Path(root)
        self.sequence_length, self.phase, self.occ, self.N, self.with_semantic = sequence_length, phase, occ, N, with_semantic
        seq_ids = list(range(-int(sequence_length / 2), int(sequence_length / 2) + 1))
        seq_ids.remove(0)
        self.seq_ids = [x + 10 for x in seq_ids]

    def paths(self, index):
        name = str(index).zfill(6)
        multiview = self.root / 'data_scene_flow_multiview' / self.phase / 'image_2'
        flow = self.root / 'data_scene_flow' / self.phase
        return {'tgt': multiview / (name + '_10.png'),
                'ref': [multiview / (name + '_' + str(k).zfill(2) + '.png') for k in self.seq_ids],
                'flow': flow / self.occ / (name + '_10.png'),
                'calib': self.root / 'data_scene_flow_calib' / self.phase / 'calib_cam_to_cam' / (name + '.txt'),
                'obj_map': flow / 'obj_map' / (name + '_10.png'),
                'semantic': self.root / 'semantic_labels' / self.phase / 'semantic' / (name + '_10.png')}

    def __getitem__(self, index):
        if not 0 <= index < self.N:
            raise IndexError(index)
        p = self.paths(index)
        tgt = imread(p['tgt'])
        obj_map = _imread_gray(p['obj_map']) if p['obj_map'].is_file() else np.ones(tgt.shape[:2], dtype=np.uint8)
        P_rect = np.reshape(read_raw_calib_file(p['calib'])['P_rect_02'], (3, 4))
        return {'tgt': tgt, 'ref': [imread(r) for r in p['ref']], 'intrinsics': P_rect[:, :3].astype('float32'),
                'flow_path': p['flow'], 'obj_map': obj_map,
                'semantic': _imread_gray(p['semantic']) if self.with_semantic else None, 'paths': p}

    def __len__(self):
        return self.N


def scale_intrinsics(intrinsics, in_hw, out_hw):
    """custom_transforms.Scale's intrinsics (custom_transforms.py:133-134) in float32 and np.linalg.inv of the result"""
    K = np.copy(np.asarray(intrinsics, dtype=np.float32))
    K[0] *= (out_hw[1] / in_hw[1])
    K[1] *= (out_hw[0] / in_hw[0])
    return K, np.linalg.inv(K)


def kitti2015_item(sample, img_hw, frames_dev, with_flow=True):
    """One Kitti2015Flow item as the reference's loader hands it to the loop at batch size 1 (Scale(h, w), ArrayToTensor,
    Normalize; test_flow.py:78-85): -> (tgt_img [1,3,h,w], ref_imgs, intrinsics [1,3,3], intrinsics_inv, flow_gt [1,3,Hg,Wg] or
    None, obj_map_gt [1,Hg,Wg] fp32, semantic uint8 [Hg,Wg] or None), all on frames_dev's device.  Scale ALWAYS calls imresize
    (custom_transforms.py:135), so every float frame is byte-scaled to its own min..max even at an equal size; the resize, the
    division by 255 and the normalisation run on the device (DeviceFrames.resize_crop)."""
    from .custom_transforms import _bytescale
    dev = frames_dev.device
    frames = [sample['tgt']] + list(sample['ref'])
    u8 = np.stack([_bytescale(np.asarray(f, dtype=np.float32)) for f in frames])
    x = frames_dev.resize_crop(u8, tuple(img_hw), tuple(img_hw))
    K, Kinv = scale_intrinsics(sample['intrinsics'], sample['tgt'].shape[:2], img_hw)
    flow_gt = read_flow_png(sample['flow_path'], dev)[None] if with_flow else None
    obj_map = torch.from_numpy(np.ascontiguousarray(sample['obj_map'], dtype=np.float32)).to(dev)[None]
    sem = None
    if sample['semantic'] is not None:
        sem = torch.from_numpy(np.where(np.asarray(sample['semantic']) == 26, 26, 0).astype(np.uint8)).to(dev)
    return (x[:1], [x[k:k + 1] for k in range(1, x.shape[0])], torch.from_numpy(K).to(dev)[None],
            torch.from_numpy(Kinv).to(dev)[None], flow_gt, obj_map, sem)


# ---------------------------------------------------------------------------------------------------------- evaluation loops
def _device_of(net):
    return next(net.parameters()).device


def _pose_of(out):
    """PoseExpNet returns (exp_mask, pose), PoseNetB6 / PoseNet6 the pose alone"""
    return out[1] if isinstance(out, (tuple, list)) else out


def _net_input(frames_dev, imgs, img_hw, no_resize):
    """test_disp.py:82-101 / test_pose.py:49-66 for N frames of one size: imresize of the float frame (byte-scaled to its own
    min..max first, as scipy.misc.imresize does for a float array) when the size differs from img_hw, then /255, -0.5, /0.5;
    -> fp32 [N,3,h,w] on the device."""
    from .custom_transforms import _bytescale
    H, W = imgs[0].shape[:2]
    if not no_resize and (H, W) != tuple(img_hw):
        u8 = np.stack([_bytescale(np.asarray(f, dtype=np.float32)) for f in imgs])
        return frames_dev.resize_crop(u8, tuple(img_hw), tuple(img_hw))
    return frames_dev(np.stack([np.asarray(f) for f in imgs]))


def evaluate_depth(disp_net, framework, min_depth=1e-3, max_depth=80, pose_net=None, spatial_normalize=False, img_hw=(256, 832),
                   no_resize=False):
    """test_disp.py:main without argparse over a KittiRawEigen framework -> (mean_errors [2,7] fp64 numpy, ERROR_NAMES).
    Row 1 is the median-scaled table of the paper; row 0 the PoseNet-scaled one (zeros without pose_net).  The framework's
    seq_length must give pose_net.nb_ref_imgs reference frames.

    pose_net may be a PoseExpNet, which returns (exp_mask, pose), or a PoseNetB6 / PoseNet6, which return the pose alone.  The
    reference's `_, poses = pose_net(...)` (test_disp.py:129) fails for the latter at batch size 1; here both work.

    Per image the frames are normalised (and resized) on the device, the ground truth comes from cc_velo_depth, the prediction
    1/disp is zoomed to its size by cc_spline_zoom and scored by cc_eigen_errors into a device buffer; the host reads that buffer
    once, after the loop.  The per-image errors are fp64 (the reference stores them as fp32)."""
    from . import loss_functions as LF
    from .custom_transforms import DeviceFrames
    dev = _device_of(disp_net)
    disp_net.eval()
    if pose_net is not None:
        pose_net.eval()
    frames_dev = DeviceFrames(device=dev)
    n = len(framework)
    errors = torch.zeros((max(n, 1), 2, 7), dtype=torch.float64, device=dev)
    with torch.no_grad():
        for j in range(n):
            sample = framework[j]
            imgs = [sample['tgt']] + (list(sample['ref']) if pose_net is not None else [])
            x = _net_input(frames_dev, imgs, img_hw, no_resize)
            tgt = x[:1]
            pred_disp = disp_net(tgt)
            if spatial_normalize:
                pred_disp = LF.spatial_normalize(pred_disp)
            pred_depth = 1 / pred_disp[0, 0]                                             # :121
            H, W = sample['tgt'].shape[:2]
            gt = velo_depth(torch.from_numpy(sample['velo']).to(dev), torch.from_numpy(sample['P_velo2im']).to(dev), H, W)
            zoomed = spline_zoom(pred_depth, H, W, min_depth, max_depth)                 # :125
            disp_t = norm = None
            if pose_net is not None:
                poses = _pose_of(pose_net(tgt, [x[k:k + 1] for k in range(1, x.shape[0])]))
                norm = poses[0, :, :3].norm(2, 1)                                        # :130
                disp_t = torch.from_numpy(np.asarray(sample['displacements'], dtype=np.float64))
            eigen_errors(gt, zoomed, min_depth, max_depth, disp_t, norm, out=errors[j])
    err = errors[:n].cpu().numpy()                                                       # the one host read-back
    return err.mean(0), list(ERROR_NAMES)


def evaluate_pose(pose_net, framework, rotation_mode='euler', img_hw=(256, 832), no_resize=False, batch_size=8):
    """test_pose.py:main without argparse over a KittiOdometry framework.  Snippets go through the network batch_size at a time
    (the tgt frame is the middle one, test_pose.py:58-63), then one cc_pose_snippet_errors launch per sequence; the host reads
    the errors once, after the loop.  -> dict with
      'errors'      [n_snippets, 2] fp64 (ATE, RE) per snippet, sequences in framework order;
      'per_snippet' {'mean', 'std'} over the snippets;
      'reference'   {'mean', 'std'} as test_pose.py:93-94 prints them: the reference sizes its error array by the framework's
                    __len__, which counts frames, not snippets (pose_evaluation_utils.py:33-34), so its statistics include
                    2 * demi_length zero rows per sequence.  Use these to compare with published numbers;
      'names'       POSE_ERROR_NAMES."""
    from .custom_transforms import DeviceFrames
    dev = _device_of(pose_net)
    pose_net.eval()
    frames_dev = DeviceFrames(device=dev)
    L, step = framework.seq_length, framework.step
    mid = L // 2
    errs = []
    with torch.no_grad():
        for seq in framework.sequences:
            first = seq['first']
            S = len(first)
            if S == 0:
                continue
            pred = torch.empty((S, L - 1, 6), dtype=torch.float32, device=dev)
            for b0 in range(0, S, batch_size):
                b1 = min(S, b0 + batch_size)
                ids = [[int(first[s]) + i * step for i in range(L)] for s in range(b0, b1)]
                uniq = sorted({f for row in ids for f in row})
                pos = {f: k for k, f in enumerate(uniq)}
                x = _net_input(frames_dev, [imread(seq['img_files'][f]) for f in uniq], img_hw, no_resize)
                snip = [x[torch.tensor([pos[row[i]] for row in ids], device=dev)] for i in range(L)]
                pred[b0:b1] = _pose_of(pose_net(snip[mid], snip[:mid] + snip[mid + 1:]))
            gt = torch.from_numpy(seq['poses']).to(dev)
            errs.append(pose_snippet_errors(pred, gt, torch.from_numpy(first), rotation_mode, step))
    E = torch.cat(errs).cpu().numpy() if errs else np.zeros((0, 2))                     # the one host read-back
    return dict(errors=E, names=list(POSE_ERROR_NAMES), per_snippet=pose_statistics(E),
                reference=pose_statistics(E, framework.n_frames))


def pose_statistics(errors, n_rows=None):
    """mean / std (population, as np.std) of per-snippet errors [n,2]; with n_rows, over errors padded with zero rows to n_rows
    as test_pose.py:44,93-94 does."""
    E = np.asarray(errors, dtype=np.float64).reshape(-1, 2)
    if n_rows is not None and n_rows > E.shape[0]:
        E = np.concatenate([E, np.zeros((n_rows - E.shape[0], 2))])
    if E.shape[0] == 0:
        return {'mean': np.full(2, math.nan), 'std': np.full(2, math.nan)}
    return {'mean': E.mean(0), 'std': E.std(0)}


def evaluate_flow(disp_net, pose_net, mask_net, flow_net, framework, THRESH=0.01, flownet='Back2Future', img_hw=(256, 832), store=None,
                  batch_size=1):
    """test_flow.py:main without argparse over a Kitti2015Flow framework -> (errors [8] fp64 numpy, FLOW_ERROR_NAMES): EPE of
    the composed flow over all / static / moving pixels and Fl, with the predicted rigidity mask and with the ground-truth object
    map.  test_flow.py:108-146 is the loop of train.py:650-748 statement for statement (and has no spatial_normalize), so the
    items go through validate.validate_flow_with_gt unchanged: one launch for the composition, one for the eight errors, one
    host read-back after the loop.  The ground-truth PNG is inflated on the host and unfiltered on the device.

    store: a `datasets.FlowValStore` of the framework (`FlowValStore.build(framework, img_hw, device)`, or loaded from its cache):
    the pass then reads no file -- `framework` may be None -- and goes through validate.validate_flow_from_store, batch_size
    samples per forward pass.  Without a store, batch_size must be 1 (the ground truths differ in size)."""
    from . import validate as V
    from .custom_transforms import DeviceFrames
    args = types.SimpleNamespace(THRESH=THRESH, flownet=flownet, spatial_normalize=False)
    if store is not None:
        errors, _ = V.validate_flow_from_store(store, disp_net, pose_net, mask_net, flow_net, batch_size=batch_size, args=args)
        return np.asarray(errors, dtype=np.float64), list(FLOW_ERROR_NAMES)
    if batch_size != 1:
        raise ValueError("evaluate_flow: batch_size %d needs a FlowValStore (store=)" % batch_size)
    frames_dev = DeviceFrames(device=_device_of(disp_net))

    def items():
        for i in range(len(framework)):
            yield kitti2015_item(framework[i], img_hw, frames_dev)[:6]

    errors, _ = V.validate_flow_with_gt(items(), disp_net, pose_net, mask_net, flow_net, args=args)
    return np.asarray(errors, dtype=np.float64), list(FLOW_ERROR_NAMES)


def mask_sample_outputs(disp_net, pose_net, mask_net, flow_net, item, flownet='Back2Future'):
    """test_mask.py:119-127 for one loader item: the four forward passes and pose2flow -> (explainability_mask, flow_cam,
    flow_fwd)"""
    from .inverse_warp import pose2flow
    tgt_img, ref_imgs, intrinsics, intrinsics_inv = item[:4]
    depth = 1 / disp_net(tgt_img)
    pose = _pose_of(pose_net(tgt_img, ref_imgs))
    explainability_mask = mask_net(tgt_img, ref_imgs)
    if flownet == 'Back2Future':
        flow_fwd = flow_net(tgt_img, ref_imgs[1:3])[0]
    else:
        flow_fwd = flow_net(tgt_img, ref_imgs[2])
    return explainability_mask, pose2flow(depth.squeeze(1), pose[:, 2], intrinsics, intrinsics_inv), flow_fwd


def evaluate_mask(disp_net, pose_net, mask_net, flow_net, framework, THRESH=0.94, flownet='Back2Future', img_hw=(256, 832)):
    """test_mask.py:main without argparse over a Kitti2015Flow framework built with_semantic=True -> dict with 'full', 'census'
    and 'bare' = (iou, bg_iou, fg_iou) of the combined, the census-only and the bare MaskNet mask (fp64, from the counts summed
    over the data set as test_mask.py:199-209), 'counts' [3,6] int64 (MASK_ROWS x MASK_COUNT_NAMES) and 'names'.

    Per sample: four forward passes, pose2flow, cc_rigidity_compose_norm and one cc_mask_iou_counts launch that adds the 18
    counts into one device buffer; the host reads that buffer once, after the loop.  Samples go one at a time, as in the
    reference, whose .max() (test_mask.py:131) spans the batch."""
    from .custom_transforms import DeviceFrames
    nets = (disp_net, pose_net, mask_net, flow_net)
    for net in nets:
        net.eval()
    dev = _device_of(disp_net)
    frames_dev = DeviceFrames(device=dev)
    counts = torch.zeros((3, 6), dtype=torch.int64, device=dev)
    with torch.no_grad():
        for i in range(len(framework)):
            sample = framework[i]
            assert sample['semantic'] is not None, "evaluate_mask: build the framework with with_semantic=True"
            item = kitti2015_item(sample, img_hw, frames_dev, with_flow=False)
            r = rigidity_composition_norm(*mask_sample_outputs(*nets, item, flownet), THRESH,
                                          want=("rigidity_mask", "rigidity_mask_census", "rigidity_mask_combined"))
            mask_iou_counts((item[5][0] != 0).to(torch.uint8), item[6],
                            (r.rigidity_mask_combined[0, 0], r.rigidity_mask_census[0, 0], r.rigidity_mask[0, 0]), counts)
    c = counts.cpu().numpy()                                                             # the one host read-back
    out = mask_ious(c)
    out.update(counts=c, names=list(MASK_COUNT_NAMES))
    return out


# ---------------------------------------------------------------------------------------------------------------- command line
def _load(name, path, dev, **kw):
    from . import models
    weights = torch.load(path, map_location='cpu')
    net = getattr(models, name)(**kw)
    net.load_state_dict(weights['state_dict'], strict=False)
    return net.to(dev), weights


def _seq_length(path):
    return int(torch.load(path, map_location='cpu')['state_dict']['conv1.0.weight'].size(1) / 3)


def _depth_main(args):
    dev = torch.device('cuda')
    disp_net, _ = _load(args.dispnet, args.pretrained_dispnet, dev)
    pose_net, seq_length = None, 0
    if args.pretrained_posenet is None:
        print('no PoseNet specified, scale_factor will be determined by median ratio')
    else:
        seq_length = _seq_length(args.pretrained_posenet)
        kw = dict(nb_ref_imgs=seq_length - 1)
        if args.posenet == 'PoseExpNet':
            kw['output_exp'] = False
        pose_net, _ = _load(args.posenet, args.pretrained_posenet, dev, **kw)
    test_files = read_text_lines(args.dataset_list)
    framework = KittiRawEigen(args.dataset_dir, test_files, seq_length, args.min_depth, args.max_depth)
    print('{} files to test'.format(len(test_files)))
    mean_errors, names = evaluate_depth(disp_net, framework, args.min_depth, args.max_depth, pose_net, args.spatial_normalize,
                                        (args.img_height, args.img_width), args.no_resize)
    if pose_net is not None:
        print("Results with scale factor determined by PoseNet : ")
        print("{:>10}, {:>10}, {:>10}, {:>10}, {:>10}, {:>10}, {:>10}".format(*names))
        print("{:10.4f}, {:10.4f}, {:10.4f}, {:10.4f}, {:10.4f}, {:10.4f}, {:10.4f}".format(*mean_errors[0]))
    print("Results with scale factor determined by GT/prediction ratio (like the original paper) : ")
    print("{:>10}, {:>10}, {:>10}, {:>10}, {:>10}, {:>10}, {:>10}".format(*names))
    print("{:10.4f}, {:10.4f}, {:10.4f}, {:10.4f}, {:10.4f}, {:10.4f}, {:10.4f}".format(*mean_errors[1]))


def _pose_main(args):
    dev = torch.device('cuda')
    seq_length = _seq_length(args.pretrained_posenet)
    pose_net, _ = _load(args.posenet, args.pretrained_posenet, dev, nb_ref_imgs=seq_length - 1)
    framework = KittiOdometry(args.dataset_dir, args.sequences, seq_length)
    print('{} snippets to test'.format(len(framework)))
    res = evaluate_pose(pose_net, framework, args.rotation_mode, (args.img_height, args.img_width), args.no_resize)
    print('')
    print("Results")
    print("\t {:>10}, {:>10}".format(*res['names']))
    print("mean \t {:10.4f}, {:10.4f}".format(*res['reference']['mean']))
    print("std \t {:10.4f}, {:10.4f}".format(*res['reference']['std']))
    print("per snippet (without the reference's zero rows)")
    print("mean \t {:10.4f}, {:10.4f}".format(*res['per_snippet']['mean']))
    print("std \t {:10.4f}, {:10.4f}".format(*res['per_snippet']['std']))


def _four_nets(args, dev):
    """test_flow.py:87-99 / test_mask.py:86-98"""
    disp_net, _ = _load(args.dispnet, args.pretrained_disp, dev)
    pose_net, _ = _load(args.posenet, args.pretrained_pose, dev, nb_ref_imgs=4)
    mask_net, _ = _load(args.masknet, args.pretrained_mask, dev, nb_ref_imgs=4)
    flow_net, _ = _load(args.flownet, args.pretrained_flow, dev, nlevels=args.nlevels)
    return disp_net, pose_net, mask_net, flow_net


def _flow_store(args, framework, dev):
    """the resident store of --batch-size / --cache: loaded from the cache directory when it holds one, else built (and saved)"""
    import os
    from .datasets import FlowValStore
    if args.cache is not None and os.path.isfile(os.path.join(args.cache, "store.json")):
        store = FlowValStore.load(args.cache, device=dev)
        if len(store) != len(framework) or tuple(store.inputs.shape[3:]) != (args.img_height, args.img_width):
            raise ValueError("%s holds %d samples at %d x %d, not the %d at %d x %d asked for"
                             % (args.cache, len(store), store.inputs.shape[3], store.inputs.shape[4], len(framework), args.img_height,
                                args.img_width))
        return store
    store = FlowValStore.build(framework, (args.img_height, args.img_width), device=dev)
    if args.cache is not None:
        store.save(args.cache)
    return store


def _flow_main(args):
    dev = torch.device('cuda')
    framework = Kitti2015Flow(args.kitti_dir, sequence_length=5, N=args.N)
    store = _flow_store(args, framework, dev) if (args.cache is not None or args.batch_size != 1) else None
    errors, names = evaluate_flow(*_four_nets(args, dev), framework, args.THRESH, args.flownet, (args.img_height, args.img_width),
                                  store=store, batch_size=args.batch_size)
    print("Results")
    print("\t {:>10}, {:>10}, {:>10}, {:>6}, {:>10}, {:>10}, {:>10}, {:>10} ".format(*names))
    print("Errors \t {:10.4f}, {:10.4f}, {:10.4f}, {:10.4f}, {:10.4f}, {:10.4f}, {:10.4f}, {:10.4f}".format(*errors))


def _mask_main(args):
    dev = torch.device('cuda')
    framework = Kitti2015Flow(args.kitti_dir, sequence_length=5, N=args.N, with_semantic=True)
    res = evaluate_mask(*_four_nets(args, dev), framework, args.THRESH, args.flownet, (args.img_height, args.img_width))
    for title, key in (("Results Full Model", 'full'), ("Results Census only", 'census'), ("Results Bare", 'bare')):
        print(title)
        print("\t {:>10}, {:>10}, {:>10} ".format('iou', 'bg_iou', 'fg_iou'))
        print("Errors \t {:10.4f}, {:10.4f} {:10.4f}".format(*res[key]))


def _kitti2015_arguments(q, thresh):
    q.add_argument('--kitti-dir', dest='kitti_dir', type=str, required=True, help='Path to the kitti2015 scene flow dataset')
    q.add_argument('--dispnet', dest='dispnet', type=str, default='DispResNet6', help='depth network architecture.')
    q.add_argument('--posenet', dest='posenet', type=str, default='PoseNetB6', help='pose network architecture.')
    q.add_argument('--masknet', dest='masknet', type=str, default='MaskNet6', help='explainabity mask network architecture.')
    q.add_argument('--flownet', dest='flownet', type=str, default='Back2Future', help='flow network architecture.')
    q.add_argument('--THRESH', dest='THRESH', type=float, default=thresh, help='THRESH')
    q.add_argument('--pretrained-disp', dest='pretrained_disp', required=True, metavar='PATH', help='path to pre-trained dispnet model')
    q.add_argument('--pretrained-pose', dest='pretrained_pose', required=True, metavar='PATH', help='path to pre-trained posenet model')
    q.add_argument('--pretrained-flow', dest='pretrained_flow', required=True, metavar='PATH', help='path to pre-trained flownet model')
    q.add_argument('--pretrained-mask', dest='pretrained_mask', required=True, metavar='PATH', help='path to pre-trained masknet model')
    q.add_argument('--nlevels', dest='nlevels', type=int, default=6, help='number of levels in multiscale.')
    q.add_argument('--dataset', dest='dataset', default='kitti2015', choices=['kitti2015'])
    q.add_argument('--N', dest='N', type=int, default=200, help='number of samples (the training set holds 200)')
    q.add_argument("--img-height", default=256, type=int, help="Image height")
    q.add_argument("--img-width", default=832, type=int, help="Image width")


def parser():
    p = argparse.ArgumentParser(description='KITTI depth (Eigen split), odometry, 2015 flow and motion-segmentation evaluation on the device')
    sub = p.add_subparsers(dest='command', required=True)
    d = sub.add_parser('depth', help='test_disp.py: Eigen-split depth errors against velodyne ground truth')
    d.add_argument("--dispnet", dest='dispnet', type=str, default='DispResNet6', help='dispnet architecture')
    d.add_argument("--posenet", dest='posenet', type=str, default='PoseExpNet', help='posenet architecture')
    d.add_argument("--pretrained-dispnet", required=True, type=str, help="pretrained DispNet path")
    d.add_argument("--pretrained-posenet", default=None, type=str, help="pretrained PoseNet path (for scale factor)")
    d.add_argument("--img-height", default=256, type=int, help="Image height")
    d.add_argument("--img-width", default=832, type=int, help="Image width")
    d.add_argument("--no-resize", action='store_true', help="no resizing is done")
    d.add_argument("--spatial-normalize", action='store_true', help="spatial normalization")
    d.add_argument("--min-depth", default=1e-3, type=float)
    d.add_argument("--max-depth", default=80, type=float)
    d.add_argument("--dataset-dir", default='.', type=str, help="KITTI raw directory")
    d.add_argument("--dataset-list", required=True, type=str, help="test file list (e.g. the Eigen split's test_files_eigen.txt)")
    d.add_argument("--gt-type", default='KITTI', type=str, choices=['KITTI'], help="GroundTruth data type")
    q = sub.add_parser('pose', help='test_pose.py: odometry ATE / RE against KITTI odometry poses')
    q.add_argument("pretrained_posenet", type=str, help="pretrained PoseNet path")
    q.add_argument("--posenet", type=str, default="PoseNetB6", help="PoseNet architecture")
    q.add_argument("--img-height", default=256, type=int, help="Image height")
    q.add_argument("--img-width", default=832, type=int, help="Image width")
    q.add_argument("--no-resize", action='store_true', help="no resizing is done")
    q.add_argument("--dataset-dir", default='.', type=str, help="KITTI odometry directory")
    q.add_argument("--sequences", default=['09'], type=str, nargs='*', help="sequences to test")
    q.add_argument("--rotation-mode", default='euler', choices=['euler', 'quat'], type=str)
    f = sub.add_parser('flow', help='test_flow.py: KITTI 2015 EPE all / static / moving and Fl')
    _kitti2015_arguments(f, 0.01)
    f.add_argument('--batch-size', dest='batch_size', type=int, default=1,
                   help='samples per forward pass; above 1 the samples are kept on the device (datasets.FlowValStore)')
    f.add_argument('--cache', dest='cache', type=str, default=None, metavar='DIR',
                   help='keep the samples on the device and cache the decoded store in DIR (loaded from there when present)')
    _kitti2015_arguments(sub.add_parser('mask', help='test_mask.py: motion-segmentation IoU (full, census only, bare)'), 0.94)
    return p


def main(argv=None):
    args = parser().parse_args(argv)
    {'depth': _depth_main, 'pose': _pose_main, 'flow': _flow_main, 'mask': _mask_main}[args.command](args)


if __name__ == '__main__':
    main()
