"""Write tests/golden/prepare_kitti.npz, prepare_cityscapes.npz and prepare_test_scenes.txt: what the UNMODIFIED reference
data/prepare_train_data.py (with kitti_raw_loader.py and cityscapes_loader.py) writes for the synthetic trees of
tests/prepare_cases.py -- KITTI with the speed rule and with the static-frames list (both --with-gt), and Cityscapes.  Per run: the
relative file listing, every cam.txt text, train.txt / val.txt, every array handed to imsave, every .npy that survives the split.
prepare_test_scenes.txt is the reference's own list (names only), which its loader reads from beside itself.
Runs only where the reference tree exists (CC_REFERENCE_ROOT or the oracle's default); never in a test and never on a GPU machine.

The reference script does not run on a current stack as it is; it is served, unchanged, by stand-ins placed in sys.modules:
  path.Path          a str subclass with the dozen methods the three files use; dirs() / files() SORT (the real ones list in
                     directory order, which is why the product documents "sorted split order")
  scipy.misc         imread = Pillow's decoder, imresize = oracle/pilutil.imresize, imsave = record the array, then
                     Image.fromarray(arr).save(name) (what SciPy 1.1's imsave did)
  joblib             Parallel runs its jobs inline;  tqdm: the bare iterable;  np.int = int

    python tools/make_prepare_golden.py [golden_dir]
"""
import fnmatch
import os
import runpy
import shutil
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import prepare_cases as C  # noqa: E402
from oracle import pilutil, ref_import  # noqa: E402


class Path(str):
    def __truediv__(self, other):
        return Path(os.path.join(self, other))

    def __add__(self, other):
        return Path(str.__add__(self, other))

    name = property(lambda self: os.path.basename(self))
    parent = property(lambda self: Path(os.path.dirname(self)))

    def basename(self):
        return Path(os.path.basename(self))

    def dirname(self):
        return Path(os.path.dirname(self))

    def realpath(self):
        return Path(os.path.realpath(self))

    def isfile(self):
        return os.path.isfile(self)

    def dirs(self):
        return [self / n for n in sorted(os.listdir(self)) if os.path.isdir(os.path.join(self, n))] if os.path.isdir(self) else []

    def files(self, pattern="*"):
        return [self / n for n in sorted(os.listdir(self)) if fnmatch.fnmatchcase(n, pattern) and os.path.isfile(os.path.join(self, n))]

    def makedirs_p(self):
        os.makedirs(self, exist_ok=True)
        return self

    mkdir_p = makedirs_p

    def rmtree(self):
        shutil.rmtree(self)

    def remove_p(self):
        if os.path.exists(self):
            os.remove(self)


def run_reference(argv, saved):
    """prepare_train_data.py as __main__ with `argv`; every (path, array) handed to imsave is appended to `saved`"""
    from PIL import Image
    import scipy
    assert ref_import.reference_available(), "reference tree not present"
    data = os.path.join(ref_import.REF_ROOT, "data")

    def imsave(name, arr):
        saved.append((str(name), np.array(arr)))
        Image.fromarray(arr).save(str(name))

    mods = {"path": types.ModuleType("path"), "scipy.misc": types.ModuleType("scipy.misc"), "joblib": types.ModuleType("joblib"),
            "tqdm": types.ModuleType("tqdm")}
    mods["path"].Path = Path
    mods["scipy.misc"].imread = lambda p: np.asarray(Image.open(str(p)))
    mods["scipy.misc"].imresize = pilutil.imresize
    mods["scipy.misc"].imsave = imsave
    mods["joblib"].Parallel = lambda n_jobs=1: (lambda jobs: [f(*a, **k) for f, a, k in jobs])
    mods["joblib"].delayed = lambda f: (lambda *a, **k: (f, a, k))
    mods["tqdm"].tqdm = lambda it, *a, **k: it
    before = {k: sys.modules.get(k) for k in list(mods) + ["kitti_raw_loader", "cityscapes_loader"]}
    had_misc, had_int, argv0, path0 = getattr(scipy, "misc", None), getattr(np, "int", None), sys.argv, list(sys.path)
    sys.modules.update(mods)
    scipy.misc, np.int, sys.argv = mods["scipy.misc"], int, ["prepare_train_data.py"] + argv
    sys.path.insert(0, data)
    try:
        runpy.run_path(os.path.join(data, "prepare_train_data.py"), run_name="__main__")
    finally:
        sys.argv, sys.path[:] = argv0, path0
        for k, v in before.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
        if had_misc is None:
            del scipy.misc
        else:
            scipy.misc = had_misc
        if had_int is None:
            del np.int
        else:
            np.int = had_int


def record(run, dump, saved, out):
    """the run's entries of the archive, after the conditions the fixture has to meet"""
    names = C.listing(dump)
    train, val = C.read_text(os.path.join(dump, "train.txt")), C.read_text(os.path.join(dump, "val.txt"))
    assert train.split() and val.split(), (run, "both lists must be non-empty")
    out[run + ":listing"], out[run + ":train"], out[run + ":val"] = np.array(names), np.array(train), np.array(val)
    for n in names:
        if n.endswith("/cam.txt"):
            out["%s:cam:%s" % (run, n[:-8])] = np.array(C.read_text(os.path.join(dump, n)))
    for path, arr in saved:
        assert arr.dtype == np.uint8
        out["%s:img:%s" % (run, os.path.relpath(path, dump).replace(os.sep, "/")[:-4])] = arr
    npys = [n for n in names if n.endswith(".npy")]
    if run.startswith("kitti"):
        assert len(train.split()) + len(val.split()) >= 6
        assert npys and all(n.split("/")[0] in val.split() for n in npys), "a val scene keeps its .npy, a train scene has lost them"
        assert all(any(n.startswith(s + "/") for n in npys) for s in val.split())
        for n in npys:
            d = np.load(os.path.join(dump, n))
            assert d.dtype == np.float32 and (d > 0).mean() >= 0.25, (n, float((d > 0).mean()))
            out["%s:npy:%s" % (run, n[:-4])] = d
    else:
        assert not npys


def closest_point_rule_is_exercised(src, dump, out, run):
    """some pixel of some surviving map is hit by two or more points of different depths and holds the smallest: recomputed here
    from the tree's files with the reference's own projection (kitti_raw_loader.py:140-171)"""
    ld = C.kitti_loader(src, os.path.join(ROOT, "tests", "golden"), run)
    for key in [k for k in out if k.startswith(run + ":npy:")]:
        scene, fid = key.split(":")[2].split("/")
        rec = [s for dr in ld.scenes for s in ld.collect_scenes(dr) if s["rel_path"] == scene][0]
        pts, Pm = ld.depth_inputs(rec, fid)
        v = pts.copy()
        v[:, 3] = 1
        v = v[v[:, 0] >= 0]
        q = np.dot(Pm, v.T).T
        q[:, :2] = q[:, :2] / q[:, -1:]
        x, y = np.round(q[:, 0]) - 1, np.round(q[:, 1]) - 1
        ok = (x >= 0) & (y >= 0) & (x < ld.width) & (y < ld.height)
        pix = (y[ok] * ld.width + x[ok]).astype(np.int64)
        z = q[ok, 2]
        for p in np.unique(pix):
            zs = z[pix == p]
            if len(zs) > 1 and zs.min() != zs.max() and out[key].reshape(-1)[p] == np.float32(zs.min()) and zs[-1] != zs.min():
                return True
    return False


def main(golden_dir):
    os.makedirs(golden_dir, exist_ok=True)
    shutil.copyfile(os.path.join(ref_import.REF_ROOT, "data", "test_scenes.txt"), os.path.join(golden_dir, "prepare_test_scenes.txt"))
    work = tempfile.mkdtemp(prefix="ccprep")
    while "_" in work:                       # cityscapes_loader.py:71 splits the camera file's WHOLE path at '_'
        shutil.rmtree(work)
        work = tempfile.mkdtemp(prefix="ccprep")
    try:
        kitti = C.build_kitti_tree(os.path.join(work, "kitti"))
        city = C.build_cityscapes_tree(os.path.join(work, "city"))
        out_k, out_c = {}, {}
        for run, src, out, argv in (
                ("kitti_speed", kitti, out_k, ["--dataset-format", "kitti", "--with-gt"]),
                ("kitti_static", kitti, out_k, ["--dataset-format", "kitti", "--with-gt", "--static-frames", os.path.join(kitti, "static_frames.txt")]),
                ("cityscapes", city, out_c, ["--dataset-format", "cityscapes"])):
            dump, saved = os.path.join(work, "dump" + run.replace("_", "")), []
            hw = C.KITTI_HW if run.startswith("kitti") else C.CITY_HW
            run_reference([src] + argv + ["--dump-root", dump, "--height", str(hw[0]), "--width", str(hw[1]), "--num-threads", "1"], saved)
            record(run, dump, saved, out)
            if run.startswith("kitti"):
                assert closest_point_rule_is_exercised(src, dump, out, run), run
        np.savez_compressed(os.path.join(golden_dir, "prepare_kitti.npz"), **out_k)
        np.savez_compressed(os.path.join(golden_dir, "prepare_cityscapes.npz"), **out_c)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    for n in ("prepare_kitti.npz", "prepare_cityscapes.npz", "prepare_test_scenes.txt"):
        print("wrote %s (%d bytes)" % (n, os.path.getsize(os.path.join(golden_dir, n))))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden"))
