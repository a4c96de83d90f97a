"""Write tests/golden/kitti_eval.npz: the reference's KITTI evaluation outputs for the seeded inputs of
tests/kitti_eval_cases.py.  Runs only where the reference tree exists (CC_REFERENCE_ROOT or the oracle's default); never in a
test and never on a GPU machine.

The functions are lifted with `ast` from the UNMODIFIED reference files, as oracle/make_golden.py:reference_train_functions
does: generate_depth_map, read_calib_file, load_velodyne_points, sub2ind, generate_mask (kitti_eval/depth_evaluation_utils.py),
compute_errors (test_disp.py), compute_pose_error (test_pose.py) and pose_vec2mat with euler2mat / quat2mat (inverse_warp.py).
They run with `np.int = int` (removed in NumPy 1.24) and a scipy.misc stand-in in scope; the zoom is scipy.ndimage.zoom itself.
The main-loop lines of test_disp.py / test_pose.py are restated below, with their line numbers.

    python tools/make_kitti_eval_golden.py [out.npz]
"""
import ast
import os
import pathlib
import sys
import tempfile
import types
from collections import Counter

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import kitti_eval_cases as C  # noqa: E402
from oracle import ref_import  # noqa: E402


def lift(relpath, names, ns):
    tree = ast.parse(open(os.path.join(ref_import.REF_ROOT, relpath)).read())
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert sorted(n.name for n in fns) == sorted(names), (relpath, [n.name for n in fns])
    exec(compile(ast.Module(body=fns, type_ignores=[]), "reference/" + relpath, "exec"), ns)


def reference_functions():
    misc = types.ModuleType("scipy.misc")           # the scripts' scipy.misc.imread / imresize (gone since SciPy 1.3): unused here
    misc.imread = misc.imresize = None
    ns = dict(np=np, torch=torch, Counter=Counter, Path=pathlib.Path, imread=misc.imread, imresize=misc.imresize)
    lift("kitti_eval/depth_evaluation_utils.py",
         ["generate_depth_map", "read_calib_file", "load_velodyne_points", "sub2ind", "generate_mask"], ns)
    lift("test_disp.py", ["compute_errors"], ns)
    lift("test_pose.py", ["compute_pose_error"], ns)
    lift("inverse_warp.py", ["euler2mat", "quat2mat", "pose_vec2mat"], ns)
    return ns


def write_calib(d, W, H):
    cam2cam, velo2cam = C.calib(W, H)
    fmt = lambda a: " ".join(repr(float(x)) for x in a)          # noqa: E731
    with open(d / "calib_cam_to_cam.txt", "w") as f:
        f.write("calib_time: 09-Jan-2012 13:57:47\n")
        for k, v in cam2cam.items():
            f.write("%s: %s\n" % (k, fmt(v)))
    with open(d / "calib_velo_to_cam.txt", "w") as f:
        f.write("calib_time: 15-Mar-2012 11:37:16\n")
        f.write("R: %s\nT: %s\n" % (fmt(velo2cam["R"]), fmt(velo2cam["T"])))


def main(out):
    ns = reference_functions()
    np.int = int                                    # generate_depth_map's .astype(np.int)
    g = {}
    with tempfile.TemporaryDirectory() as tmp:
        tmp = pathlib.Path(tmp)
        for name, H, W, n, seed in C.VELO_CASES:
            pts = C.velo_points(H, W, n, seed)
            d = tmp / name
            d.mkdir()
            write_calib(d, W, H)
            pts.tofile(str(d / "velo.bin"))
            depth = ns["generate_depth_map"](d, d / "velo.bin", (H, W), 2)
            cal = ns["read_calib_file"](d / "calib_cam_to_cam.txt")
            assert np.array_equal(cal["P_rect_02"], C.calib(W, H)[0]["P_rect_02"])
            idx = np.flatnonzero(depth)
            g["velo_%s_idx" % name] = idx.astype(np.int32)
            g["velo_%s_val" % name] = depth.reshape(-1)[idx].astype(np.float32)
            # the Eigen mask of this map (generate_mask, :194-206), as flat indices
            g["velo_%s_mask" % name] = np.flatnonzero(ns["generate_mask"](depth, 1e-3, 80)).astype(np.int32)
    for name, h, w, H, W, seed in C.ZOOM_CASES:
        from scipy.ndimage import zoom
        src = C.zoom_source(h, w, seed)
        z = zoom(src, (H / src.shape[0], W / src.shape[1])).clip(1e-3, 80)     # test_disp.py:125
        assert z.shape == (H, W) and z.dtype == np.float32
        if H * W <= 64 * 256:
            g[name] = z
        else:
            rows, cols = C.zoom_keep(H, W)
            g[name + "_rows"] = z[rows]
            g[name + "_cols"] = np.ascontiguousarray(z[:, cols])
    for name, even, seed in (("e_even", True, 14), ("e_odd", False, 15)):
        gt, pred, disp, norm = C.eigen_case(seed, even=even)
        gt_depth = gt.astype(np.float64)
        mask = ns["generate_mask"](gt_depth, 1e-3, 80)
        assert (mask.sum() % 2 == 0) == even
        p, gd = pred[mask], gt_depth[mask]                       # :126-128
        e = np.zeros((2, 7))
        scale_factors = [s1 / s2 for s1, s2 in zip(disp, norm) if s1 > 0]                     # :133-134
        e[0] = ns["compute_errors"](gd, p * np.mean(scale_factors))                           # :137
        e[1] = ns["compute_errors"](gd, p * (np.median(gd) / np.median(p)))                  # :139-140
        g[name] = e
    for name, L, mode, S, seed in C.POSE_CASES:
        pred, seq, first = C.pose_case(L, S, seed)
        err, fin = np.zeros((S, 2)), np.zeros((S, L, 3, 4))
        for s in range(S):
            poses = torch.from_numpy(pred[s])                                                  # test_pose.py:73-76
            poses = torch.cat([poses[:L // 2], torch.zeros(1, 6).float(), poses[L // 2:]])
            inv_transform_matrices = ns["pose_vec2mat"](poses, rotation_mode=mode).numpy().astype(np.float64)  # :78
            rot_matrices = np.linalg.inv(inv_transform_matrices[:, :, :3])                    # :80-86
            tr_vectors = -rot_matrices @ inv_transform_matrices[:, :, -1:]
            transform_matrices = np.concatenate([rot_matrices, tr_vectors], axis=-1)
            first_inv_transform = inv_transform_matrices[0]
            final_poses = first_inv_transform[:, :3] @ transform_matrices
            final_poses[:, :, -1:] += first_inv_transform[:, -1:]
            gp = np.stack([seq[i] for i in first[s] + np.arange(L)])                         # pose_evaluation_utils.py:19-23
            first_pose = gp[0]
            gp[:, :, -1] -= first_pose[:, -1]
            compensated_poses = np.linalg.inv(first_pose[:, :3]) @ gp
            err[s] = ns["compute_pose_error"](compensated_poses, final_poses)
            fin[s] = final_poses
        g[name + "_err"] = err
        g[name + "_final"] = fin
    np.savez_compressed(out, **g)
    print("wrote %s (%d arrays, %d bytes)" % (out, len(g), os.path.getsize(out)))


if __name__ == "__main__":
    assert ref_import.reference_available(), "the reference tree is needed to write the fixture"
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "kitti_eval.npz"))
