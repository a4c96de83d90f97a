"""Write tests/golden/validation_folder.json: the frame and depth-file order the UNMODIFIED reference datasets/validation_folders.py
(`ValidationSet`) gives on the synthetic tree of tests/validation_store_cases.py.  Names only.
Runs only where the reference tree exists (CC_REFERENCE_ROOT or the oracle's default); never in a test and never on a GPU machine.

The reference module imports `path.Path` and `scipy.misc.imread`; both are served by the stand-ins of tools/make_sequence_golden.py
(its `Path` extended by the three more methods this module calls).
The reference reads each line of val.txt as `line[:-1]`, which presumes the newline: on a list whose last line has none it cuts the
scene's last letter and finds no folder.  The fixture is therefore written from the same tree with the newline present; the test
runs on the tree without it, where the product must give the same order.

    python tools/make_validation_golden.py [out.json]
"""
import importlib.util
import json
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)
import validation_store_cases as C  # noqa: E402
from make_sequence_golden import Path as _Path  # noqa: E402
from oracle import ref_import  # noqa: E402


class Path(_Path):
    """the sequence tool's stand-in plus what validation_folders.py also calls: dirname(), .name, isfile()"""

    def __truediv__(self, other):
        return Path(os.path.join(self, other))

    def files(self, pattern):
        return [Path(p) for p in _Path.files(self, pattern)]

    def dirname(self):
        return Path(os.path.dirname(self))

    @property
    def name(self):
        return os.path.basename(self)

    def isfile(self):
        return os.path.isfile(self)


def load_reference():
    from PIL import Image
    assert ref_import.reference_available(), "reference tree not present"
    path_mod = types.ModuleType("path")
    path_mod.Path = Path
    misc = types.ModuleType("scipy.misc")
    misc.imread = lambda p: np.asarray(Image.open(p))
    saved = {k: sys.modules.get(k) for k in ("path", "scipy.misc")}
    sys.modules["path"], sys.modules["scipy.misc"] = path_mod, misc
    try:
        spec = importlib.util.spec_from_file_location("ccref_validation_folders", os.path.join(ref_import.REF_ROOT, "datasets", "validation_folders.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod


def main(out):
    ref = load_reference()
    with tempfile.TemporaryDirectory() as d:
        root = C.build_val_tree(os.path.join(d, "val"), final_newline=True)
        ds = ref.ValidationSet(root)
        gold = {"scenes": C.rel_names(root, ds.scenes), "imgs": C.rel_names(root, ds.imgs), "depth": C.rel_names(root, ds.depth)}
        assert len(ds) == len(gold["imgs"]) == len(gold["depth"])
        # the reference's own decode of one item, against Pillow and the stored depth (what the tests compare the product with)
        img, depth = ds[1]
        from frame_store_cases import pillow_float
        assert img.dtype == np.float32 and np.array_equal(img, pillow_float(ds.imgs[1]))
        assert depth.dtype == np.float32 and np.array_equal(depth, np.load(ds.depth[1]).astype(np.float32))
    with open(out, "w") as f:
        json.dump(gold, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "validation_folder.json"))
