#!/usr/bin/env python3
"""GPU box: one untraced forward per node-encoder route case on a sparse ring graph, to be run under a kernel trace once per library
build (GNNCCA_LIB=...), and the reduction of such a trace to one line per launch -- the A/B of two builds' LAUNCHES, where
tools/hash_logits.py is the A/B of their bits.

    rocprofv3 --kernel-trace --output-format csv -d <dir> -- python3 tools/sweep_encoder_routes.py [--set steps]
    python3 tools/sweep_encoder_routes.py [--set steps] --reduce <dir>/**/*kernel_trace.csv > profiles/<name>.txt

The cases are those of tests/test_encoder_route.py that fit a quick run: the shipped encoder (2048 -> 128 -> 32) on both sides of every
threshold up to 8193 nodes, the deep encoders [128, 64] and [128, 128, 64] up to 8197, and 51233 nodes once.  Every case ends with a
marker launch (torch's erfinv, which nothing else here uses), so the reduced list names the case each launch belongs to.  The reduced line is
`case kernel grid workgroup lds`: two builds launch the same kernels iff their lists are equal line for line.

`--set steps`: the rows of tests/test_step_route.py that a quick untraced forward reaches -- the shipped dims on rings of `deg` edges per
node: the f32 / bf16-split message on either side of 512 nodes, the general kernel (max aggregation, reattach flags), one / two / four
waves per node, two nodes per wave and deferred classification around 16 384 nodes with 1 / 2 / 3 classifying steps, the bf16 edge
state, column ranges, the padded layout at 2^19 edges, L = 0 and L = 1.  The forced-policy rows (GNNCCA_* switches) stay on the CPU."""
import csv
import os
import re
import sys

SHIPPED = [1, 64, 320, 321, 640, 641, 2559, 2560, 4095, 4096, 8192, 8193]
DEEP = [64, 301, 1229, 3007, 4099, 8197]
CASES = [([128], n) for n in SHIPPED] + [([128, 64], n) for n in DEEP] + [([128, 128, 64], n) for n in DEEP] + [([128, 64], 51233)]
# --set steps: (nodes, edges per node, steps, classifying steps, what else)
STEPS = [(64, 63, 4, 2, ""), (512, 3, 4, 2, ""), (513, 3, 4, 2, ""), (513, 3, 4, 2, "max"), (513, 3, 4, 2, "reattach_edges"),
         (513, 3, 4, 2, "reattach_nodes"), (600, 64, 4, 2, ""), (600, 65, 4, 2, ""), (600, 192, 4, 2, ""), (600, 193, 4, 2, ""),
         (2048, 260, 4, 2, ""), (4097, 260, 4, 2, ""), (4095, 260, 4, 2, "unsplit"), (4096, 260, 4, 2, "unsplit"), (16383, 3, 4, 2, ""),
         (16384, 3, 4, 2, ""), (16384, 3, 4, 1, ""), (16384, 3, 4, 3, ""), (16384, 129, 4, 2, ""), (16384, 3, 4, 2, "bf16"),
         (16384, 3, 4, 2, "ranges"), (64, 63, 4, 2, "ranges"), (513, 3, 4, 2, "ranges"), (513, 3, 1, 1, "ranges"), (16384, 32, 4, 2, ""),
         (513, 3, 0, 1, ""), (513, 3, 1, 1, ""), (513, 3, 4, 4, ""), (16384, 3, 4, 4, "")]
MARKER = "erfinv"


def step_label(c):
    return "steps-%dx%d-L%d-C%d%s" % (c[0], c[1], c[2], c[3], "-" + c[4] if c[4] else "")


def reduce_trace(paths, labels):
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
            for ln in pending:
                print(f"{labels[case]} {ln}")
            case, pending = case + 1, []
    assert case == len(labels), f"{case} markers seen, {len(labels)} cases run"


def sweep(steps):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "tests")]
    import numpy as np
    import torch
    from test_gpu_encoder_shapes import _model
    from test_gpu_workspace_poison import _model as step_model
    from test_gpu_workspace_poison import _params, ring_graph, to_device
    models = {}
    mark = torch.zeros(64, device="cuda")
    torch.cuda.synchronize()
    mark.erfinv_()   # marker 0
    torch.cuda.synchronize()
    for case in (STEPS if steps else CASES):
        if steps:
            n, deg, L, cls, what = case
            params, arch = _params(num_enc_steps=L, num_class_steps=cls)
            if what == "max":
                params["node_agg_fn"] = "max"
            elif what.startswith("reattach"):
                params["reattach_initial_" + what.split("_")[1]] = True
            m = step_model(params, arch, seed=1)
            m.edge_state_dtype, m.encoder_unsplit, m.column_ranges = "bf16" if what == "bf16" else "fp32", what == "unsplit", what == "ranges"
            d = to_device(*ring_graph(n, np.random.default_rng(n), hops=tuple(range(1, deg + 1))))
            label = step_label(case)
        else:
            fc, n = case
            if tuple(fc) not in models:
                models[tuple(fc)] = _model(2048, fc, seed=1)[3]
            m = models[tuple(fc)]
            d = to_device(*ring_graph(n, np.random.default_rng(n)))
            label = f"{'-'.join(map(str, fc))}@{n}"
        torch.cuda.synchronize()
        with torch.no_grad():
            out = m(d)["classified_edges"]
        torch.cuda.synchronize()
        mark.erfinv_()
        torch.cuda.synchronize()
        print(f"{label} max|logit| {float(out[-1].abs().max()):.6g}", flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    steps = args[:2] == ["--set", "steps"]
    args = args[2:] if steps else args
    if len(args) > 1 and args[0] == "--reduce":
        reduce_trace(args[1:], [step_label(c) for c in STEPS] if steps else [f"{'-'.join(map(str, fc))}@{n}" for fc, n in CASES])
    else:
        sweep(steps)
