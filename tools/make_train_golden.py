"""Write tests/golden/train_args.json: the command-line options of the UNMODIFIED reference train.py (train.py:34-135), read off
its source -- the file is parsed, never imported: every `parser.add_argument(...)` call of the module is walked with `ast` and its
arguments are `literal_eval`-ed (`type=float` and friends are names: kept as the name).  Per option: option strings, dest (argparse's
own rule where none is given), type name, default, choices, action and required; no help text.
Runs only where the reference tree exists (CC_REFERENCE_ROOT or the oracle's default); never in a test and never on a GPU machine.

    python tools/make_train_golden.py [out.json]
"""
import ast
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_import  # noqa: E402


def _dest(strings):
    """argparse._get_optional_kwargs / _get_positional_kwargs: the first long option string, else the first short one"""
    if not strings[0].startswith("-"):
        return strings[0]
    longs = [s for s in strings if s.startswith("--")]
    return (longs[0][2:] if longs else strings[0][1:]).replace("-", "_")


def read_options(path):
    tree = ast.parse(open(path).read())
    out = []
    for node in ast.walk(tree):
        if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "add_argument"
                and isinstance(node.func.value, ast.Name) and node.func.value.id == "parser"):
            continue
        strings = [ast.literal_eval(a) for a in node.args]
        kw = {}
        for k in node.keywords:
            if k.arg in ("help", "metavar"):
                continue
            kw[k.arg] = k.value.id if (k.arg == "type" and isinstance(k.value, ast.Name)) else ast.literal_eval(k.value)
        action = kw.get("action", "store")
        default = kw.get("default", False if action == "store_true" else None)
        out.append((node.lineno, {"strings": strings, "dest": kw.get("dest", _dest(strings)), "type": kw.get("type"),
                                  "default": default, "choices": kw.get("choices"), "action": action,
                                  "required": bool(kw.get("required", False))}))
    return [o for _, o in sorted(out, key=lambda t: t[0])]


def main(out):
    assert ref_import.reference_available(), "reference tree not present"
    opts = read_options(os.path.join(ref_import.REF_ROOT, "train.py"))
    assert len(opts) > 50 and opts[0]["strings"] == ["data"]
    with open(out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(o, sort_keys=True) for o in opts) + "\n]\n")
    print("wrote %s (%d options, %d bytes)" % (out, len(opts), os.path.getsize(out)))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "train_args.json"))
