#!/usr/bin/env python3
"""GPU box: one untraced forward per node-encoder route case on a sparse ring graph, to be run under a kernel trace once per library
build (GNNCCA_LIB=...), and the reduction of such a trace to one line per launch -- the A/B of two builds' LAUNCHES, where
tools/hash_logits.py is the A/B of their bits.

    rocprofv3 --kernel-trace --output-format csv -d <dir> -- python3 tools/sweep_encoder_routes.py
    python3 tools/sweep_encoder_routes.py --reduce <dir>/**/*kernel_trace.csv > profiles/<name>.txt

The cases are those of tests/test_encoder_route.py that fit a quick run: the shipped encoder (2048 -> 128 -> 32) on both sides of every
threshold up to 8193 nodes, the deep encoders [128, 64] and [128, 128, 64] up to 8197, and 51233 nodes once.  Every case ends with a
marker launch (torch's erfinv, which nothing else here uses), so the reduced list names the case each launch belongs to.  The reduced line is
`case kernel grid workgroup lds`: two builds launch the same kernels iff their lists are equal line for line."""
import csv
import os
import re
import sys

SHIPPED = [1, 64, 320, 321, 640, 641, 2559, 2560, 4095, 4096, 8192, 8193]
DEEP = [64, 301, 1229, 3007, 4099, 8197]
CASES = [([128], n) for n in SHIPPED] + [([128, 64], n) for n in DEEP] + [([128, 128, 64], n) for n in DEEP] + [([128, 64], 51233)]
MARKER = "erfinv"


def reduce_trace(paths):
    rows = []
    for p in paths:
        rows += list(csv.DictReader(open(p)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    case, pending, seen_first = 0, [], False
    for r in rows:
        name = re.sub(r"\(.*", "", r["Kernel_Name"]).replace("void ", "")
        grid = "x".join(r[f"Grid_Size_{a}"] for a in "XYZ")
        wg = "x".join(r[f"Workgroup_Size_{a}"] for a in "XYZ")
        if "gnncca::" in name:
            pending.append(f"{name} {grid} {wg} {r['LDS_Block_Size']}")
            continue
        if MARKER in r["Kernel_Name"]:
            if not seen_first:   # marker 0 opens the sweep: what came before it is the set-up
                seen_first, pending = True, []
                continue
            fc, n = CASES[case]
            for ln in pending:
                print(f"{'-'.join(map(str, fc))}@{n} {ln}")
            case, pending = case + 1, []
    assert case == len(CASES), f"{case} markers seen, {len(CASES)} cases run"


def sweep():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "tests")]
    import numpy as np
    import torch
    from test_gpu_encoder_shapes import _model
    from test_gpu_workspace_poison import ring_graph, to_device
    models = {}
    mark = torch.zeros(64, device="cuda")
    torch.cuda.synchronize()
    mark.erfinv_()   # marker 0
    torch.cuda.synchronize()
    for fc, n in CASES:
        if tuple(fc) not in models:
            models[tuple(fc)] = _model(2048, fc, seed=1)[3]
        m = models[tuple(fc)]
        d = to_device(*ring_graph(n, np.random.default_rng(n)))
        torch.cuda.synchronize()
        with torch.no_grad():
            out = m(d)["classified_edges"]
        torch.cuda.synchronize()
        mark.erfinv_()
        torch.cuda.synchronize()
        print(f"{'-'.join(map(str, fc))}@{n} max|logit| {float(out[-1].abs().max()):.6g}", flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--reduce":
        reduce_trace(sys.argv[2:])
    else:
        sweep()
