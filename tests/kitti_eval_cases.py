"""Seeded inputs of the KITTI evaluation tests (tests/test_kitti_eval.py) and of the fixture generator
tools/make_kitti_eval_golden.py, which records the reference's outputs for them in tests/golden/kitti_eval.npz.

Velodyne cases use a calibration whose products and sums are exact in double (dyadic values: P_rect with f = 64 and a
principal point on quarter pixels, an axis-permuting velo->cam rotation, T = (0, 0, -1/2)), so that points planted exactly on
a .5 rounding tie give the same tie whatever the summation order of the reference's dot product."""
import numpy as np

F_PX = 64.0

# (name, H, W, n random points, seed): a small image, KITTI's 375x1242 and the 376x1241 of the 2011_10_03 drives
VELO_CASES = [("small", 24, 40, 300, 1), ("kitti", 375, 1242, 4000, 2), ("kitti_1241", 376, 1241, 3000, 3)]
# (name, h, w, H, W, seed): reduced sizes kept whole, KITTI sizes kept as border rows / columns
ZOOM_CASES = [("z_small", 16, 40, 23, 61, 4), ("z_mid", 32, 104, 47, 155, 5), ("z_kitti", 256, 832, 375, 1242, 6),
              ("z_1241", 256, 832, 376, 1241, 7), ("z_1224", 256, 832, 370, 1224, 8), ("z_1238", 256, 832, 374, 1238, 9)]
# (name, L, rotation mode, S, seed)
POSE_CASES = [("p3_euler", 3, "euler", 6, 10), ("p5_euler", 5, "euler", 5, 11), ("p5_quat", 5, "quat", 5, 12),
              ("p3_quat", 3, "quat", 4, 13)]


def calib(W, H):
    """-> (calib_cam_to_cam dict, calib_velo_to_cam dict) of float arrays, every value exact in decimal text"""
    cx, cy = W / 2.0 + 0.25, H / 2.0 - 0.25
    P_rect = np.array([[F_PX, 0, cx, 0], [0, F_PX, cy, 0], [0, 0, 1, 0]], dtype=np.float64)
    R = np.array([[0, -1, 0], [0, 0, -1], [1, 0, 0]], dtype=np.float64)      # cam = (-y, -z, x) + T
    cam2cam = {"R_rect_00": np.eye(3).reshape(-1), "P_rect_02": P_rect.reshape(-1), "P_rect_03": P_rect.reshape(-1)}
    velo2cam = {"R": R.reshape(-1), "T": np.array([0.0, 0.0, -0.5])}
    return cam2cam, velo2cam


def P_velo2im(W, H):
    cam2cam, velo2cam = calib(W, H)
    v2c = np.vstack((np.hstack((velo2cam["R"].reshape(3, 3), velo2cam["T"][:, None])), [0, 0, 0, 1.0]))
    R = np.eye(4)
    R[:3, :3] = cam2cam["R_rect_00"].reshape(3, 3)
    return np.dot(np.dot(cam2cam["P_rect_02"].reshape(3, 4), R), v2c)


def _point_at(u_img, v_img, w, W, H):
    """velodyne (x, y, z) whose projection is exactly (u_img, v_img) before rounding, at camera depth w (dyadic)"""
    cx, cy = W / 2.0 + 0.25, H / 2.0 - 0.25
    return [w + 0.5, (cx - u_img) * w / F_PX, (cy - v_img) * w / F_PX, 0.0]


def velo_points(H, W, n, seed):
    """raw velodyne points [N,4] fp32: random points (some behind, some out of the image), same-pixel duplicates, the
    (v, W-1) / (v+1, 0) sub2ind collisions, negative camera depths and exact .5 ties."""
    r = np.random.RandomState(seed)
    w = r.uniform(1.0, 90.0, n)
    u = r.uniform(-0.2 * W, 1.2 * W, n)
    v = r.uniform(-0.2 * H, 1.2 * H, n)
    cx, cy = W / 2.0 + 0.25, H / 2.0 - 0.25
    pts = np.stack([w + 0.5, (cx - u) * w / F_PX, (cy - v) * w / F_PX, r.rand(n)], 1)
    pts[r.rand(n) < 0.05, 0] *= -1                                       # behind the sensor: dropped (x < 0)
    planted = []
    for k in range(max(4, n // 50)):
        i = r.randint(n)                                                  # same pixel, other depths (and a negative one)
        for d in (0.5, 2.0, -0.25):
            planted.append([pts[i, 0] * d + 0.5 * (1 - d), pts[i, 1] * d, pts[i, 2] * d, 0.5])
    for k in range(8):                                                    # sub2ind collisions: (v, W-1) and (v+1, 0)
        vv = 1 + r.randint(H - 2)
        ws = [2.0 ** r.randint(0, 6), 2.0 ** r.randint(0, 6), 0.25]
        planted.append(_point_at(W - 1 + 1, vv + 1, ws[0], W, H))         # u-1 = W-1, v-1 = vv
        planted.append(_point_at(0 + 1, vv + 2, ws[1], W, H))             # u-1 = 0, v-1 = vv+1
        if k % 2:
            planted.append(_point_at(W - 1 + 1, vv + 1, -ws[2], W, H))    # negative depth at the same key
        else:
            planted.append(_point_at(0 + 1, vv + 2, ws[2], W, H))
    for k in range(24):                                                   # exact .5 ties in u and in v, even and odd
        uu = 1 + r.randint(W - 2) + 0.5
        vv = 1 + r.randint(H - 2) + (0.5 if k % 2 else 0.0)
        planted.append(_point_at(uu, vv, 2.0 ** r.randint(-1, 6), W, H))
    planted.append(_point_at(W + 1.0, 3.0, 4.0, W, H))                    # just outside: u-1 = W
    planted.append(_point_at(3.0, 0.0, 4.0, W, H))                        # just outside: v-1 = -1
    allp = np.concatenate([pts, np.array(planted)]).astype(np.float32)
    return allp[r.permutation(len(allp))]


def zoom_source(h, w, seed):
    """a positive fp32 depth-like prediction [h,w] (1 / sigmoid-range disparities)"""
    r = np.random.RandomState(seed)
    return (1.0 / (r.rand(h, w) * 0.3 + 0.01)).astype(np.float32)


def zoom_keep(H, W):
    """the rows and columns of a KITTI-size zoom that the fixture stores: two at each border"""
    return np.array([0, 1, H - 2, H - 1]), np.array([0, 1, W - 2, W - 1])


def eigen_case(seed, H=60, W=100, even=True):
    """fp32 ground truth (sparse, some beyond max_depth) and prediction [H,W] with an even (or odd) number of valid pixels,
    plus displacements / pose norms for the PoseNet row (one displacement 0)."""
    r = np.random.RandomState(seed)
    gt = np.where(r.rand(H, W) < 0.4, r.uniform(0.5, 95.0, (H, W)), 0.0).astype(np.float32)
    crop = np.array([0.40810811 * H, 0.99189189 * H, 0.03594771 * W, 0.96405229 * W]).astype(np.int32)
    ok = np.zeros((H, W), bool)
    ok[crop[0]:crop[1], crop[2]:crop[3]] = True
    ok &= (gt > 1e-3) & (gt < 80)
    if (ok.sum() % 2 == 0) != even:
        y, x = np.argwhere(ok)[0]
        gt[y, x] = 0.0
    pred = (gt * r.uniform(0.3, 0.5, (H, W)) + r.uniform(0.5, 5.0, (H, W))).astype(np.float32)
    disp = np.array([1.25, 0.0, 0.75, 1.5])
    norm = r.uniform(0.05, 0.2, 4).astype(np.float32)
    return gt, pred, disp, norm


def pose_case(L, S, seed):
    """network poses [S,L-1,6] fp32 and a raw sequence [F,3,4] fp64 with first [S] (snippets at step 1)"""
    r = np.random.RandomState(seed)
    F = S + L + 2
    pred = np.concatenate([r.randn(S, L - 1, 3) * 0.5, r.randn(S, L - 1, 3) * 0.1], 2).astype(np.float32)
    ang = r.randn(F, 3) * 0.2
    seq = np.zeros((F, 3, 4))
    for f in range(F):
        a, b, c = ang[f]
        Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
        Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
        Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
        seq[f, :, :3] = Rx @ Ry @ Rz
        seq[f, :, 3] = np.array([0.1, -0.05, 1.0]) * f + r.randn(3) * 0.2
    first = np.sort(r.choice(F - L + 1, S, replace=False)).astype(np.int32)
    return pred, seq, first
