"""Static guard for the code paths the CPU suite cannot execute (hipGraph capture, multi-GPU bench legs): every global
name the product modules, bench.py and __graft_entry__.py load must be defined somewhere in that module."""
import ast
import builtins
import glob
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _undefined(path):
    tree = ast.parse(open(path).read())
    defined = set(dir(builtins)) | {"__file__", "__name__", "__doc__"}
    for n in ast.walk(tree):
        if isinstance(n, (ast.Import, ast.ImportFrom)):
            for a in n.names:
                defined.add((a.asname or a.name).split(".")[0])
        elif isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)):
            defined.add(n.name)
            if not isinstance(n, ast.ClassDef):
                a = n.args
                for x in a.posonlyargs + a.args + a.kwonlyargs:
                    defined.add(x.arg)
                for x in (a.vararg, a.kwarg):
                    if x is not None:
                        defined.add(x.arg)
        elif isinstance(n, ast.Lambda):
            for x in n.args.args:
                defined.add(x.arg)
        elif isinstance(n, ast.Name) and isinstance(n.ctx, (ast.Store, ast.Del)):
            defined.add(n.id)
        elif isinstance(n, ast.ExceptHandler) and n.name:
            defined.add(n.name)
    return sorted({n.id for n in ast.walk(tree) if isinstance(n, ast.Name) and isinstance(n.ctx, ast.Load) and n.id not in defined})


def test_no_undefined_names():
    files = glob.glob(os.path.join(ROOT, "cc_amd", "*.py")) + glob.glob(os.path.join(ROOT, "cc_amd", "models", "*.py")) + \
        [os.path.join(ROOT, "bench.py"), os.path.join(ROOT, "__graft_entry__.py")]
    bad = {os.path.relpath(f, ROOT): u for f in files for u in [_undefined(f)] if u}
    assert not bad, bad


# the entry points of the launcher families of cc_amd/ops.py (conv forward / data gradient, activation backward + bias sums,
# batch norm, x2 up-sampling, the 9x9 cost volume): each is spelled out -- name and argument list -- in exactly one place
LAUNCHER_ENTRIES = ["cc_conv2d_fwd", "cc_conv2d_fwd_group", "cc_conv2d_dgrad", "cc_conv2d_dgrad_group", "cc_conv2d_dgrad_group_add",
                    "cc_act_bwd_bias_group", "cc_act_bwd_bias_group_defer", "cc_bn_train_fwd", "cc_bn_train_bwd", "cc_bn_eval_fwd",
                    "cc_upsample2x_fwd", "cc_upsample2x_bwd", "cc_corr9x9_fwd", "cc_corr9x9_bwd"]


def test_launcher_entries_are_spelled_once():
    import re
    src = {os.path.relpath(f, ROOT): open(f).read() for f in glob.glob(os.path.join(ROOT, "cc_amd", "*.py"))}
    sites = {}
    for f, text in src.items():
        for m in re.finditer(r"\bcall\(\s*[\"'](cc_\w+)[\"']", text):
            sites.setdefault(m.group(1), []).append(f)
    for name in LAUNCHER_ENTRIES:
        assert sites.get(name) == ["cc_amd/ops.py"], (name, sites.get(name))
    assert not any("_Conv2dFn" in text for text in src.values())
