"""Write tests/golden/sequence_folder.json: the sample order and the intrinsics the UNMODIFIED reference datasets/sequence_folders.py
gives on the synthetic tree of tests/frame_store_cases.py, for seeds {0, 3} and sequence lengths {3, 5}.  Names and numbers only.
Runs only where the reference tree exists (CC_REFERENCE_ROOT or the oracle's default); never in a test and never on a GPU machine.

The reference module imports `path.Path` (not installed) and `scipy.misc.imread` (gone since SciPy 1.3): both are served by small
stand-ins placed in sys.modules -- a str subclass with `/` and `.files(pattern)`, and Pillow's decoder.

    python tools/make_sequence_golden.py [out.json]
"""
import fnmatch
import importlib.util
import json
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import frame_store_cases as C  # noqa: E402
from oracle import ref_import  # noqa: E402


class Path(str):
    def __truediv__(self, other):
        return Path(os.path.join(self, other))

    def files(self, pattern):
        return [self / n for n in os.listdir(self) if fnmatch.fnmatchcase(n, pattern) and os.path.isfile(os.path.join(self, n))]


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
        spec = importlib.util.spec_from_file_location("ccref_sequence_folders", os.path.join(ref_import.REF_ROOT, "datasets", "sequence_folders.py"))
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
    gold = {"seeds": list(C.SEEDS), "sequence_lengths": list(C.LENGTHS), "order": {}, "intrinsics": {}}
    with tempfile.TemporaryDirectory() as d:
        root = C.build_tree(os.path.join(d, "tree"))
        for seed in C.SEEDS:
            for L in C.LENGTHS:
                ds = ref.SequenceFolder(root, seed=seed, train=True, sequence_length=L)
                gold["order"]["seed%d.len%d" % (seed, L)] = [C.rel_names(root, [s["tgt"]] + s["ref_imgs"]) for s in ds.samples]
                for s in ds.samples:
                    scene = os.path.basename(os.path.dirname(s["tgt"]))
                    K = [[float(v) for v in row] for row in s["intrinsics"]]
                    assert s["intrinsics"].dtype == np.float32 and gold["intrinsics"].setdefault(scene, K) == K
                # the reference's own decode of one sample, against Pillow (what the tests compare the product with)
                tgt, refs, K, Kinv = ds[0]
                assert np.array_equal(tgt, C.pillow_float(ds.samples[0]["tgt"])) and np.array_equal(Kinv, np.linalg.inv(K))
    with open(out, "w") as f:
        json.dump(gold, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "sequence_folder.json"))
