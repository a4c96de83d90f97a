"""KITTI evaluation on the device: Eigen-split depth (reference test_disp.py with kitti_eval/depth_evaluation_utils.py) and
odometry ATE / RE (test_pose.py with kitti_eval/pose_evaluation_utils.py).

Thin wrappers over the HIP entries of cc_amd/csrc/kitti_eval.hip (include/ccengine.h, "KITTI evaluation"), the two evaluation
loops, dataset readers that mirror the reference's metadata code on `pathlib` and PIL, and a command line:

    python -m cc_amd.kitti_eval depth --pretrained-dispnet D.pth.tar [--pretrained-posenet P.pth.tar] --dataset-dir RAW \\
        --dataset-list test_files_eigen.txt
    python -m cc_amd.kitti_eval pose P.pth.tar --dataset-dir ODOMETRY --sequences 09 10

The ground-truth depth map, the spline zoom of the prediction, the masked median scaling and the errors all run as kernels; the
evaluation loops read results back to the host once, after the loop.  Readers return what the files hold (uint8 frames, raw
velodyne points, P_velo2im, displacements, ground-truth poses); no depth map is built on the host.
"""
import argparse
import datetime
import math
import pathlib

import numpy as np
import torch

from ._lib import engine, STREAM

ERROR_NAMES = ['abs_rel', 'sq_rel', 'rms', 'log_rms', 'a1', 'a2', 'a3']       # test_disp.py:144
POSE_ERROR_NAMES = ['ATE', 'RE']                                               # test_pose.py:96
ROTATION_MODES = {'euler': 0, 'quat': 1}


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


def parser():
    p = argparse.ArgumentParser(description='KITTI depth (Eigen split) and odometry evaluation on the device')
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
    return p


def main(argv=None):
    args = parser().parse_args(argv)
    if args.command == 'depth':
        _depth_main(args)
    else:
        _pose_main(args)


if __name__ == '__main__':
    main()
