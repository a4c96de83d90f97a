"""Write tests/golden/kitti_flow_eval.npz: the reference's KITTI 2015 mask-evaluation outputs for the seeded inputs of
tests/kitti_flow_cases.py.  Runs only where the reference tree exists (CC_REFERENCE_ROOT or the oracle's default); never in a
test and never on a GPU machine.

`mask_error` is lifted with `ast` from the UNMODIFIED test_mask.py, as tools/make_kitti_eval_golden.py and
oracle/make_golden.py:reference_train_functions do, with scipy.ndimage.zoom as its `zoom`.  The composition statements of
main()'s loop body (test_mask.py:129-138) are lifted as AST nodes by line number and executed on the synthetic tensors; the
.cpu().data[0].numpy() conversions (:143-148) and the three mask_error calls (:150-152) are restated below with their line numbers.

The masks are stored bit-packed.  The tool asserts that every one of the 18 counts is non-zero and that each mask has a mean
between 0.05 and 0.95, and that scipy's zoom(order=0) is the index lookup ccengine.h documents for cc_mask_iou_counts.

flow_read_png (flowutils/flow_io.py:96-117) needs pypng and cannot run here; its two arithmetic lines (:114-115) are restated in
tests/kitti_flow_np.py:flow_from_bytes, and the decoder is pinned by the PNG tests (an encoder's input, Pillow's high bytes, a
byte-wise restatement of the PNG specification).

    python tools/make_kitti_flow_golden.py [out.npz]
"""
import ast
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import kitti_flow_cases as C  # noqa: E402
import kitti_flow_np as R  # noqa: E402
from oracle import ref_import  # noqa: E402

FIRST_LINE, LAST_LINE = 129, 138
NAMES = ("rigidity_mask", "rigidity_mask_census_soft", "rigidity_mask_census", "rigidity_mask_combined", "flow_fwd_non_rigid",
         "flow_fwd_rigid", "total_flow")


def reference_functions():
    from scipy.ndimage import zoom
    tree = ast.parse(open(os.path.join(ref_import.REF_ROOT, "test_mask.py")).read())
    ns = dict(np=np, torch=torch, zoom=zoom)
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "mask_error"]
    assert len(fns) == 1
    exec(compile(ast.Module(body=fns, type_ignores=[]), "reference/test_mask.py", "exec"), ns)
    main = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "main"][0]
    loop = [n for n in main.body if isinstance(n, ast.For)][0]
    stmts = [n for n in loop.body if FIRST_LINE <= n.lineno <= LAST_LINE]
    got = [n.targets[0].id for n in stmts if isinstance(n, ast.Assign)]
    assert len(got) == len(stmts) and tuple(dict.fromkeys(got)) == NAMES, got
    ns["_compose_code"] = compile(ast.Module(body=stmts, type_ignores=[]), "reference/test_mask.py:129-138", "exec")
    return ns


def check_zoom_is_the_lookup(h, w, Hg, Wg, seed):
    from scipy.ndimage import zoom
    p = np.random.RandomState(seed).rand(h, w).astype(np.float32)
    z = zoom(p, (float(Hg) / float(h), float(Wg) / float(w)), order=0)         # test_mask.py:234-237
    assert z.shape == (Hg, Wg) and np.array_equal(z, R.zoom_nearest(p, Hg, Wg)), (h, w, Hg, Wg)


def save_npz(out, arrays):
    """np.savez_compressed with fixed member timestamps and a fixed order, so that the same arrays give the same bytes"""
    with zipfile.ZipFile(out, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main(out):
    ns = reference_functions()
    g = {}
    for name, h, w, Hg, Wg, seed in C.MASK_CASES:
        check_zoom_is_the_lookup(h, w, Hg, Wg, seed)
        mask, cam, fwd = C.compose_inputs(h, w, seed)
        obj, sem = C.gt_maps(Hg, Wg, seed)
        loc = dict(explainability_mask=torch.from_numpy(mask), flow_cam=torch.from_numpy(cam), flow_fwd=torch.from_numpy(fwd),
                   args=types.SimpleNamespace(THRESH=C.THRESH))
        exec(ns["_compose_code"], loc)
        rigidity_mask_combined_np = loc["rigidity_mask_combined"].cpu().data[0].numpy()         # :143
        rigidity_mask_census_np = loc["rigidity_mask_census"].cpu().data[0].numpy()             # :144
        rigidity_mask_bare_np = loc["rigidity_mask"].cpu().data[0].numpy()                      # :145
        gt_mask_np = torch.LongTensor(obj.astype(np.int64))[None][0].numpy()                    # validation_flow.py:168, :147
        semantic_map_np = torch.LongTensor(sem.astype(np.int64))[None][0].numpy()               # validation_flow.py:169, :148
        counts = np.array([ns["mask_error"](gt_mask_np, semantic_map_np, rigidity_mask_combined_np[0]),      # :150
                           ns["mask_error"](gt_mask_np, semantic_map_np, rigidity_mask_census_np[0]),        # :151
                           ns["mask_error"](gt_mask_np, semantic_map_np, rigidity_mask_bare_np[0])])         # :152
        assert counts.shape == (3, 6) and np.all(counts > 0), counts
        assert np.all(counts == np.round(counts))
        for key, m in (("combined", rigidity_mask_combined_np), ("census", rigidity_mask_census_np), ("bare", rigidity_mask_bare_np)):
            m = np.asarray(m, dtype=np.float32).reshape(h, w)
            assert np.all((m == 0) | (m == 1)) and 0.05 < m.mean() < 0.95, (name, key, m.mean())
            g["%s_%s" % (name, key)] = np.packbits(m.astype(np.uint8).reshape(-1))
        g["%s_counts" % name] = counts.astype(np.int64)
        # the masked flows of the small case, whole
        if h * w <= 4096:
            for key in ("flow_fwd_non_rigid", "flow_fwd_rigid", "total_flow"):
                g["%s_%s" % (name, key)] = loc[key].numpy()
    save_npz(out, g)
    print("wrote %s (%d arrays, %d bytes)" % (out, len(g), os.path.getsize(out)))
    assert os.path.getsize(out) < 300 * 1024


if __name__ == "__main__":
    assert ref_import.reference_available(), "the reference tree is needed to write the fixture"
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "kitti_flow_eval.npz"))
