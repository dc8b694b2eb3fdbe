#!/usr/bin/env python3
"""Register / scratch / occupancy table of the kernels in libgnncca_mpn (compile-only, runs without a GPU).
usage: python tools/kernel_regs.py [substring ...]     e.g.  python tools/kernel_regs.py mpn_step_pipe_kernel"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gnn-cca_amd"))
import build  # noqa: E402  (the library's source list)

out = "/tmp/gnncca_regs.txt"
if "--reuse" not in sys.argv or not os.path.exists(out):
    units = [s for s in build.SOURCES if s.endswith(".hip")]   # every kernel is compiled in exactly one of them
    procs = []
    for u in units:   # side by side, as build.py compiles them
        cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-x", "hip", "-I", os.path.join(ROOT, "include"), "-I",
               build.CSRC, "-DGNNCCA_BUILD", "-mllvm", "-amdgpu-mfma-vgpr-form", "--cuda-device-only", "-c", os.path.join(build.CSRC, u),
               "-o", "/tmp/gnncca_dev_%s.o" % u, "-Rpass-analysis=kernel-resource-usage"]
        procs.append(subprocess.Popen(cmd, stderr=open("%s.%s" % (out, u), "w")))
    if any(p.wait() != 0 for p in procs):
        sys.exit("hipcc failed: see %s.*" % out)
    with open(out, "w") as f:
        for u in units:
            f.write(open("%s.%s" % (out, u)).read())
want = [a for a in sys.argv[1:] if not a.startswith("--")]
rows, cur = {}, None
for line in open(out):
    m = re.search(r"Function Name: (\S+)", line)
    if m:
        cur = m.group(1)
        rows[cur] = {}
        continue
    m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
    if m and cur:
        rows[cur][m.group(1).strip()] = int(m.group(2))
names = list(rows)
dem = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.splitlines()
for n, d in zip(names, dem):
    short = d.replace("void gnncca::", "").split("(")[0]
    if want and not any(w in short for w in want):
        continue
    r = rows[n]
    print(f"{short:95s} VGPR {r.get('VGPRs'):4d} SGPR {r.get('TotalSGPRs'):4d} scratch {r.get('ScratchSize'):4d} spillV {r.get('VGPRs Spill'):3d} "
          f"spillS {r.get('SGPRs Spill'):3d} occ {r.get('Occupancy')}")
