"""Packs the same parameters with two builds of libgnncca_mpn.so and compares the blobs byte for byte; optionally times the host packer
of both, alternated.

    python tools/pack_blob_diff.py OLD/libgnncca_mpn.so NEW/libgnncca_mpn.so [--time 200]

The matrix is every golden case plus the synthetic configurations of tests/pack_configs.py (the generic golden cases go through
pack_generic).  Exit status 1 if any pair of blobs differs.  CPU only: gnncca_pack_weights is a host function."""
import argparse
import copy
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import pack_configs  # noqa: E402
from conftest import GOLDEN_DIR, golden_cases  # noqa: E402
from gnn_cca_amd import MOTMPNet, _native as nat  # noqa: E402
from oracle.mpn_oracle import load_case  # noqa: E402


def load(path):
    lib = C.CDLL(os.path.abspath(path))
    lib.gnncca_packed_weights_bytes.restype = C.c_size_t
    lib.gnncca_packed_weights_bytes.argtypes = [C.POINTER(nat.MpnDims)]
    lib.gnncca_pack_weights.restype = C.c_int
    lib.gnncca_pack_weights.argtypes = [C.POINTER(nat.MpnDims), C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_size_t]
    return lib


def models():
    for name in golden_cases():
        params, arch, sd, _ = load_case(os.path.join(GOLDEN_DIR, name + ".npz"))
        m = MOTMPNet(copy.deepcopy(params), None, arch)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
        yield "golden/" + name, m.eval()
    for name in pack_configs.NAMES:
        yield "synthetic/" + name, pack_configs.build(name)


def packer(lib, m):
    d = m.native_dims()
    host = [t.detach().to("cpu", torch.float32).contiguous() for t in m.native_param_tensors()]
    ptrs = (C.c_void_p * len(host))(*[t.data_ptr() for t in host])
    nbytes = lib.gnncca_packed_weights_bytes(C.byref(d))
    blob = np.full(nbytes, 0xA5, dtype=np.uint8)   # the packer must write every byte

    def run():
        status = lib.gnncca_pack_weights(C.byref(d), ptrs, len(host), blob.ctypes.data, nbytes)
        assert status == 0, status
        return blob
    run.keep = host
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--time", type=int, default=0, help="time the host packer on golden/terrace32 (the shipped shape): calls per library")
    a = ap.parse_args()
    old, new = load(a.old), load(a.new)
    bad = 0
    for name, m in models():
        b0, b1 = packer(old, m)(), packer(new, m)()
        same = b0.size == b1.size and np.array_equal(b0, b1)
        diff = "" if same else f"  first difference at byte {int(np.flatnonzero(b0 != b1)[0]) if b0.size == b1.size else -1}"
        print(f"{'same' if same else 'DIFFERENT':9s} {b0.size:9d} B  {name}{diff}")
        bad += not same
    print(f"{bad} differing blobs")
    if a.time:
        m = dict(models())["golden/terrace32"]
        runs = {"old": packer(old, m), "new": packer(new, m)}
        t = {"old": [], "new": []}
        for i in range(a.time + 5):
            for k in ("old", "new") if i % 2 == 0 else ("new", "old"):
                t0 = time.perf_counter()
                runs[k]()
                if i >= 5:
                    t[k].append((time.perf_counter() - t0) * 1e3)
        for k in ("old", "new"):
            q = statistics.quantiles(t[k], n=10)
            print(f"host pack {k}: median {statistics.median(t[k]):.3f} ms, p10 {q[0]:.3f}, p90 {q[-1]:.3f}, min {min(t[k]):.3f} ({len(t[k])} calls)")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
