#!/usr/bin/env python
"""What the host planners of a library build answer, over a sweep of convolution geometries (no GPU needed).

  python tools/plan_sweep.py --lib A.so [--lib B.so] [--sets nets,parity,grid] [--write-fixture tests/golden/conv_plans.json]

Per geometry: the weight-gradient workspace (cc_conv2d_wgrad_ws_bytes) and the kernel names of the weight-gradient, forward and
data-gradient calls (cc_conv2d_{wgrad,fwd,dgrad}_kernel) -- host-only entry points, loaded with ctypes.  With two libraries the
answers are compared row by row (exit status 1 on any difference); --write-fixture records the answers of the first library for
the `nets` and `parity` sets (tests/test_abi.py holds the library to that file, so a planner edit shows up as a fixture diff).

Sets: nets = every Conv2d / ConvTranspose2d layer of the four networks at the three sizes of tests/test_headline_gpu.py;
parity = CONV_CASES* / CONVT_CASES / WGRAD_LIST_SHAPES* of tests/parity.py; grid = channels x map sizes x kernel sizes x strides."""
import argparse
import ctypes
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

COLUMNS = ["wgrad_ws_bytes", "wgrad_kernel", "fwd_kernel", "dgrad_kernel", "dgrad_kernel_prepacked"]


def net_layers():
    """(kind, B, Cin, H, W, Cout, k, stride, pad, output_padding) of every convolution the step runs at the benchmarked sizes"""
    import torch
    from cc_amd import synthetic as syn
    from oracle import step as S
    from oracle.make_golden import HEADLINE
    seen = []

    def hook(m, inp, out):
        x = inp[0]
        kind = "convT" if isinstance(m, torch.nn.ConvTranspose2d) else "conv"
        assert m.kernel_size[0] == m.kernel_size[1] and m.stride[0] == m.stride[1] and m.padding[0] == m.padding[1] and m.groups == 1
        row = (kind, x.shape[0], m.in_channels, x.shape[2], x.shape[3], m.out_channels, m.kernel_size[0], m.stride[0], m.padding[0],
               m.output_padding[0] if kind == "convT" else 0)
        if row not in seen:
            seen.append(row)

    for _, full, B, H, W in HEADLINE:
        nets = S.build_nets("oracle", flow=full, mask=full)
        hs = [m.register_forward_hook(hook) for n in nets if n is not None for m in n.modules()
              if isinstance(m, (torch.nn.Conv2d, torch.nn.ConvTranspose2d))]
        with torch.no_grad():
            S.cc_forward(nets, syn.sample(B, H, W, seed=1), S.StepConfig())
        for h in hs:
            h.remove()
    return seen


def parity_cases():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import parity
    rows = []
    for name in sorted(vars(parity)):
        v = getattr(parity, name)
        if name.startswith("CONV_CASES_WINO_ACT"):       # (B, Cin, H, W, C1, C2, ...): two 3x3 / stride-1 layers in a row
            rows += [("conv", c[0], cin, c[2], c[3], cout, 3, 1, 1, 0) for c in v for cin, cout in ((c[1], c[4]), (c[4], c[5]))]
        elif name.startswith("CONVT_CASES"):
            rows += [("convT",) + tuple(c[:9]) for c in v]
        elif name.startswith(("CONV_CASES", "WGRAD_LIST_SHAPES")):
            rows += [("conv",) + tuple(c[:8]) + (0,) for c in v]
    return list(dict.fromkeys(rows))


def grid():
    ch = (1, 2, 3, 16, 32, 47, 48, 64, 96, 128, 256, 512)
    maps = ((2, 7), (4, 13), (6, 16), (8, 26), (8, 28), (16, 52), (30, 101), (32, 104), (64, 208), (128, 416))
    return [("conv", B, cin, h, w, m, k, st, k // 2, 0)
            for m, cin, (h, w), k, st, B in itertools.product(ch, ch, maps, (1, 3, 5, 7), (1, 2), (1, 4))]


def answers(lib_path, rows):
    dll = ctypes.CDLL(lib_path)
    dll.cc_conv2d_wgrad_ws_bytes.restype = ctypes.c_size_t
    buf = ctypes.create_string_buffer(128)

    def name(fn, *a):
        assert getattr(dll, fn)(*a, buf, 128) == 0
        return buf.value.decode()

    out = []
    for kind, B, Cin, H, W, Cout, k, st, pad, opad in rows:
        if kind == "conv":
            OH, OW = (H + 2 * pad - k) // st + 1, (W + 2 * pad - k) // st + 1
            if OH < 1 or OW < 1:
                out.append(None)
                continue
            wg = (B, Cout, OH, OW, Cin, H, W, k, k, st, pad)
            out.append([dll.cc_conv2d_wgrad_ws_bytes(*wg[:5], k, k, st), name("cc_conv2d_wgrad_kernel", *wg),
                        name("cc_conv2d_fwd_kernel", B, Cin, H, W, Cout, k, k, st, pad, OH, OW),
                        name("cc_conv2d_dgrad_kernel", B, Cout, OH, OW, Cin, k, k, st, pad, H, W, 0),
                        name("cc_conv2d_dgrad_kernel", B, Cout, OH, OW, Cin, k, k, st, pad, H, W, 1)])
        else:       # transposed convolution: the weight gradient gathers dY around the pixels of the INPUT (cc_amd/ops.py)
            OH, OW = (H - 1) * st - 2 * pad + k + opad, (W - 1) * st - 2 * pad + k + opad
            wg = (B, Cin, H, W, Cout, OH, OW, k, k, st, pad)
            out.append([dll.cc_conv2d_wgrad_ws_bytes(*wg[:5], k, k, st), name("cc_conv2d_wgrad_kernel", *wg), None, None, None])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lib", action="append", required=True)
    ap.add_argument("--sets", default="nets,parity,grid")
    ap.add_argument("--write-fixture", default=None)
    a = ap.parse_args()
    sets = {"nets": net_layers, "parity": parity_cases, "grid": grid}
    rows = {s: sets[s]() for s in a.sets.split(",")}
    got = [{s: answers(lib, r) for s, r in rows.items()} for lib in a.lib]
    for s, r in rows.items():
        print("%-6s %6d geometries, %d weight-gradient kernels" % (s, len(r), len({x[1] for x in got[0][s] if x})))
    if a.write_fixture:
        fx = {"columns": ["kind", "B", "Cin", "H", "W", "Cout", "k", "stride", "pad", "output_padding"] + COLUMNS,
              "rows": [list(r) + v for s in ("nets", "parity") if s in rows for r, v in zip(rows[s], got[0][s])]}
        with open(a.write_fixture, "w") as f:
            f.write("{\"columns\": %s,\n \"rows\": [\n  %s\n ]}\n" % (json.dumps(fx["columns"]), ",\n  ".join(json.dumps(r) for r in fx["rows"])))
    bad = 0
    if len(got) > 1:
        for s, r in rows.items():
            for geom, x, y in zip(r, got[0][s], got[1][s]):
                if x != y:
                    bad += 1
                    print("DIFF %s %s\n   %s\n   %s" % (s, geom, x, y))
        print("%d difference(s)" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
