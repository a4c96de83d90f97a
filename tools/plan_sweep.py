#!/usr/bin/env python
"""What the host planners of a library build answer, over a sweep of convolution geometries (no GPU needed).

  python tools/plan_sweep.py --lib A.so [--lib B.so] [--sets nets,parity,lists,grid] [--write-fixture tests/golden/conv_plans.json]

Per geometry: the weight-gradient workspace (cc_conv2d_wgrad_ws_bytes), the kernel names of the weight-gradient, forward and
data-gradient calls (cc_conv2d_{wgrad,fwd,dgrad}_kernel) and every other host-only answer of the forward / data-gradient entry
points: workspace bytes (single call and a group of G = 3), weight-image floats and the repack descriptors (asked with source and
image address 0, so they hold offsets) -- loaded with ctypes.  With two libraries the answers are compared row by row (exit status 1
on any difference); --write-fixture records the answers of the first library for the `nets`, `parity` and `lists` sets
(tests/test_abi.py holds the library to that file, so a planner edit shows up as a fixture diff).

Sets: nets = every Conv2d / ConvTranspose2d layer of the four networks at the three sizes of tests/test_headline_gpu.py;
parity = CONV_CASES* / CONVT_CASES / WGRAD_LIST_SHAPES* of tests/parity.py; grid = channels x map sizes x kernel sizes x strides;
lists = windows of 6 consecutive `nets` layers as cc_conv2d_list records, forward and transposed arithmetic alternating
(cc_conv2d_list_ws_bytes at split targets 0 and 256)."""
import argparse
import ctypes
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

COLUMNS = ["wgrad_ws_bytes", "wgrad_kernel", "fwd_kernel", "dgrad_kernel", "dgrad_kernel_prepacked",
           "fwd_ws_bytes", "fwd_group3_ws_bytes", "dgrad_ws_bytes", "dgrad_group3_ws_bytes", "fwd_pack_floats", "dgrad_pack_floats",
           "fwd_pack_desc", "dgrad_pack_desc"]
LIST_COLUMNS = ["list_ws_bytes", "list_ws_bytes_target256"]
LIST_WINDOW = 6
CL_LONGS = 32           # longs per cc_conv2d_list record (include/ccengine.h)


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


def list_windows(layers):
    """consecutive windows of LIST_WINDOW layers -> lists of (kind of arithmetic, layer): 0 = forward, 1 = transposed, alternating"""
    return [[(j % 2, layers[i + j]) for j in range(LIST_WINDOW)] for i in range(0, len(layers) - LIST_WINDOW + 1, LIST_WINDOW)]


def _load(lib_path):
    dll = ctypes.CDLL(lib_path)
    for fn in ("cc_conv2d_wgrad_ws_bytes", "cc_conv2d_fwd_ws_bytes", "cc_conv2d_fwd_group_ws_bytes", "cc_conv2d_dgrad_ws_bytes",
               "cc_conv2d_dgrad_group_ws_bytes", "cc_conv2d_fwd_pack_floats", "cc_conv2d_dgrad_pack_floats", "cc_conv2d_list_ws_bytes"):
        getattr(dll, fn).restype = ctypes.c_size_t
    return dll


def _geometry(kind, B, Cin, H, W, Cout, k, st, pad, opad):
    """-> (forward arithmetic or None, transposed arithmetic) of a layer, each (B, channels in, h, w, channels out, k, k, st, pad, h', w'):
    a Conv2d runs forward and its data-gradient, a ConvTranspose2d the transposed arithmetic forward and a convolution backward"""
    if kind == "conv":
        OH, OW = (H + 2 * pad - k) // st + 1, (W + 2 * pad - k) // st + 1
        if OH < 1 or OW < 1:
            return None
        return (B, Cin, H, W, Cout, k, k, st, pad, OH, OW), (B, Cout, OH, OW, Cin, k, k, st, pad, H, W)
    OH, OW = (H - 1) * st - 2 * pad + k + opad, (W - 1) * st - 2 * pad + k + opad
    return (B, Cout, OH, OW, Cin, k, k, st, pad, H, W), (B, Cin, H, W, Cout, k, k, st, pad, OH, OW)


def list_answers(lib_path, windows):
    """cc_conv2d_list_ws_bytes of each window at split targets 0 (the default) and 256; the image address of every record is a
    dummy (nothing is dereferenced by the size query)"""
    dll = _load(lib_path)
    one = 0x3f800000            # act_a = 1.0f
    out = []
    for win in windows:
        recs = []
        for arith, layer in win:
            geo = _geometry(*layer)
            if geo is None:
                continue
            B, Ci, H0, W0, Co, k, _, st, pad, H1, W1 = geo[arith]
            r = [0] * CL_LONGS
            r[0], r[6] = arith, 4096
            r[8:20] = [B, Ci, H0, W0, Ci * H0 * W0, Co, k, k, st, pad, H1, W1]
            r[20], r[24] = Co * H1 * W1, one
            r[26], r[27] = Co * k * k, k * k
            recs += r
        n = len(recs) // CL_LONGS
        arr = (ctypes.c_long * len(recs))(*recs)
        out.append([dll.cc_conv2d_list_ws_bytes(n, arr, 0), dll.cc_conv2d_list_ws_bytes(n, arr, 256)])
    return out


def answers(lib_path, rows):
    dll = _load(lib_path)
    buf = ctypes.create_string_buffer(128)
    desc = (ctypes.c_long * (16 * 64))()
    L = ctypes.c_long

    def name(fn, *a):
        assert getattr(dll, fn)(*a, buf, 128) == 0
        return buf.value.decode()

    def descs(fn, *a):
        n = getattr(dll, fn)(*a, L(0), L(0), desc)
        assert 0 <= n <= 64
        return [n] + [list(desc[16 * i:16 * i + 16]) for i in range(n)]

    def sizes(fwd, tr):
        """the size / pack / descriptor columns: forward arithmetic `fwd` (or None) and transposed arithmetic `tr`"""
        ks, cs = L(tr[4] * tr[5] * tr[6]), L(tr[5] * tr[6])
        f = [None, None, None, None] if fwd is None else \
            [dll.cc_conv2d_fwd_ws_bytes(*fwd), dll.cc_conv2d_fwd_group_ws_bytes(3, *fwd), dll.cc_conv2d_fwd_pack_floats(*fwd),
             descs("cc_conv2d_fwd_pack_desc", *fwd)]
        t = [dll.cc_conv2d_dgrad_ws_bytes(*tr), dll.cc_conv2d_dgrad_group_ws_bytes(3, *tr), dll.cc_conv2d_dgrad_pack_floats(*tr, ks, cs),
             descs("cc_conv2d_dgrad_pack_desc", *tr, ks, cs)]
        return [f[0], f[1], t[0], t[1], f[2], t[2], f[3], t[3]]

    out = []
    for row in rows:
        kind, B, Cin, H, W, Cout, k, st, pad, opad = row
        if kind == "conv":
            OH, OW = (H + 2 * pad - k) // st + 1, (W + 2 * pad - k) // st + 1
            if OH < 1 or OW < 1:
                out.append(None)
                continue
            wg = (B, Cout, OH, OW, Cin, H, W, k, k, st, pad)
            out.append([dll.cc_conv2d_wgrad_ws_bytes(*wg[:5], k, k, st), name("cc_conv2d_wgrad_kernel", *wg),
                        name("cc_conv2d_fwd_kernel", B, Cin, H, W, Cout, k, k, st, pad, OH, OW),
                        name("cc_conv2d_dgrad_kernel", B, Cout, OH, OW, Cin, k, k, st, pad, H, W, 0),
                        name("cc_conv2d_dgrad_kernel", B, Cout, OH, OW, Cin, k, k, st, pad, H, W, 1)] + sizes(*_geometry(*row)))
        else:       # transposed convolution: the weight gradient gathers dY around the pixels of the INPUT (cc_amd/ops.py)
            OH, OW = (H - 1) * st - 2 * pad + k + opad, (W - 1) * st - 2 * pad + k + opad
            wg = (B, Cin, H, W, Cout, OH, OW, k, k, st, pad)
            out.append([dll.cc_conv2d_wgrad_ws_bytes(*wg[:5], k, k, st), name("cc_conv2d_wgrad_kernel", *wg), None, None, None] +
                       sizes(*_geometry(*row)))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lib", action="append", required=True)
    ap.add_argument("--sets", default="nets,parity,lists,grid")
    ap.add_argument("--write-fixture", default=None)
    a = ap.parse_args()
    sets = {"nets": net_layers, "parity": parity_cases, "grid": grid}
    names = a.sets.split(",")
    rows = {s: sets[s]() for s in names if s != "lists"}
    got = [{s: answers(lib, r) for s, r in rows.items()} for lib in a.lib]
    if "lists" in names:        # windows of the network layers
        layers = rows["nets"] if "nets" in rows else net_layers()
        rows["lists"] = list_windows(layers)
        for lib, g in zip(a.lib, got):
            g["lists"] = list_answers(lib, rows["lists"])
    for s, r in rows.items():
        if s == "lists":
            print("%-6s %6d windows of %d layers" % (s, len(r), LIST_WINDOW))
        else:
            print("%-6s %6d geometries, %d weight-gradient kernels" % (s, len(r), len({x[1] for x in got[0][s] if x})))
    if a.write_fixture:
        fx = {"columns": ["kind", "B", "Cin", "H", "W", "Cout", "k", "stride", "pad", "output_padding"] + COLUMNS,
              "rows": [list(r) + v for s in ("nets", "parity") if s in rows for r, v in zip(rows[s], got[0][s])]}
        # lists: [first row of the window (LIST_WINDOW consecutive rows, see list_windows)] + LIST_COLUMNS
        lists = [[LIST_WINDOW * i] + v for i, v in enumerate(got[0]["lists"])] if "lists" in rows and "nets" in names else []
        with open(a.write_fixture, "w") as f:
            f.write("{\"columns\": %s,\n \"rows\": [\n  %s\n ],\n \"list_columns\": %s,\n \"lists\": [\n  %s\n ]}\n" % (
                json.dumps(fx["columns"]), ",\n  ".join(json.dumps(r) for r in fx["rows"]),
                json.dumps(["first_row"] + LIST_COLUMNS), ",\n  ".join(json.dumps(r) for r in lists)))
    bad = 0
    if len(got) > 1:
        per_column = {}
        for s, r in rows.items():
            cols = LIST_COLUMNS if s == "lists" else COLUMNS
            for geom, x, y in zip(r, got[0][s], got[1][s]):
                if x != y:
                    bad += 1
                    which = [c for c, u, v in zip(cols, x or [], y or []) if u != v] or ["row"]
                    for c in which:
                        per_column[c] = per_column.get(c, 0) + 1
                    print("DIFF %s %s %s\n   %s\n   %s" % (s, geom, ",".join(which), [u for u, v in zip(x or [], y or []) if u != v],
                                                          [v for u, v in zip(x or [], y or []) if u != v]))
        print("%d difference(s)%s" % (bad, "".join("  %s: %d" % kv for kv in sorted(per_column.items()))))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
