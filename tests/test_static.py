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


# the process-wide state of a training step (cc_amd/step_scope.py): assigned, begun and ended in that module only
STEP_STATE_ASSIGNED = ["tape.BN_COUNTERS", "tape.NET_DONE", "tape.NET_MARK", "ops.grad_sinks", "wgrad_queue.enabled",
                       "LF.step_nan_flags", "LF.forward_stream"]
STEP_STATE_CALLS = ["scalar_pool.begin", "scalar_pool.end", "head_grads.begin", "head_grads.end", "packs.begin_step", "packs.end_step",
                    "packs.invalidate"]
# diagnosis: tools/branch_timeline.py wraps the installed tape.NET_DONE for the length of one network's backward call and puts
# it back (stamps around the network's tail inside a captured step)
STEP_STATE_EXCEPTIONS = {("tools/branch_timeline.py", "tape.NET_DONE")}


def _step_state_sites(root):
    """{(file, name)}: assignments (plain, augmented, chained, tuple targets) to the names above and calls of the methods above,
    matched on the dotted spelling's end (`ops.wgrad_queue.enabled = ..` is an assignment to wgrad_queue.enabled)"""
    def targets(t):
        if isinstance(t, (ast.Tuple, ast.List)):
            for e in t.elts:
                yield from targets(e)
        else:
            yield t
    sites = set()
    for f in glob.glob(os.path.join(root, "cc_amd", "*.py")) + glob.glob(os.path.join(root, "tools", "*.py")):
        rel = os.path.relpath(f, root)
        for n in ast.walk(ast.parse(open(f).read())):
            if isinstance(n, (ast.Assign, ast.AugAssign, ast.AnnAssign)):
                spelled = [ast.unparse(x) for t in (n.targets if isinstance(n, ast.Assign) else [n.target]) for x in targets(t)]
                names = STEP_STATE_ASSIGNED
            elif isinstance(n, ast.Call):
                spelled, names = [ast.unparse(n.func)], STEP_STATE_CALLS
            else:
                continue
            sites.update((rel, name) for sp in spelled for name in names if sp == name or sp.endswith("." + name))
    return sites


def test_step_state_is_switched_in_one_module():
    sites = _step_state_sites(ROOT)
    outside = {s for s in sites if s[0] != "cc_amd/step_scope.py"}
    assert outside == STEP_STATE_EXCEPTIONS, sorted(outside ^ STEP_STATE_EXCEPTIONS)
    assert {name for f, name in sites if f == "cc_amd/step_scope.py"} == set(STEP_STATE_ASSIGNED + STEP_STATE_CALLS)


# hand-rolled LDS trees deliberately left outside cc::block_tree (cc_common.h): (file, kernel) -> why
TREE_ALLOWED = {
    ("prep.hip", "k_frames_minmax_partial"): "min and max of one value in ONE barrier sequence, fminf / fmaxf (NaN-dropping) on float",
    ("prep.hip", "k_frames_minmax_final"): "the same pair over MMB = 64 partials",
    ("prep.hip", "k_store_minmax"): "min and max of one byte value in one barrier sequence, over unsigned",
    ("prep.hip", "k_local_norm_partial"): "sum and sum of squares in one barrier sequence; block_tree's order, left as it is: prep.hip is outside the consolidated kernels",
    ("prep.hip", "k_local_norm_final"): "the same pair over LNB = 64 partials",
}


def test_small_kernel_bodies_are_written_once():
    """the Adam update, the strided LDS tree and the radix-select pick each have ONE text under cc_amd/csrc/ (adam_update.h,
    cc_common.h, radix_select.h): the bit-identities between the entries that share them do not rest on copies kept alike"""
    import re
    csrc = os.path.join(ROOT, "cc_amd", "csrc")
    src = {os.path.basename(f): open(f).read() for f in glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h"))}
    assert [f for f, t in src.items() if "(1.f - b1) *" in t] == ["adam_update.h"]
    assert [f for f, t in src.items() if "st[0] |= (unsigned)j << shift" in t] == ["radix_select.h"]
    tree = re.compile(r"for\s*\(\s*(?:const\s+)?(?:int|unsigned|long|size_t)[\w\s]*?\b(\w+)\s*=[^;]+;\s*\1\s*>\s*0\s*;\s*\1\s*(?:>>=\s*1|/=\s*2)\s*\)")
    kernel = re.compile(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(")
    found = set()
    for f, t in src.items():
        if f == "cc_common.h":
            assert len(tree.findall(t)) == 1 and "block_tree" in t and "block_sum_f64" in t
            continue
        assert not re.search(r"^[^/\n]*\b\w*(block_sum|block_reduce)\w*\s*\([^;{]*\)\s*\{", t, re.M), f + " defines a block reduction of its own"
        for m in tree.finditer(t):
            owner = [k.group(1) for k in kernel.finditer(t, 0, m.start())]
            found.add((f, owner[-1] if owner else None))
    assert found == set(TREE_ALLOWED), sorted(found ^ set(TREE_ALLOWED))
