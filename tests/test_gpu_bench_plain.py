"""bench.py's plain run on hardware: ONE JSON line with the headline keys only (every other leg is behind --full), `steps` timed steps,
and `--dump-outputs` writing the logits of the timed path's last step -- bitwise the eager forward of the same seeded model and inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_plain_run_line_and_dumped_outputs(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--nodes", "64",
           "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in res, key
    assert res["steps"] == 7 and res["unit"] == "edges/s" and res["higher_is_better"] is True and res["dtype"] == "f32"
    assert res["ms_per_step"] > 0 and res["value"] > 0 and res["config"]["outputs_finite"]
    assert abs(res["value"] - 64 * 63 * 1e3 / res["ms_per_step"]) <= 1e-6 * res["value"]
    for leg in ("roofline", "kernels_us", "configs", "terrace_pipeline", "train_step", "cpu_baseline", "config4_sharded", "roofline_at_scale"):
        assert leg not in res, leg

    import bench
    model = bench.build_model(bench.graph_net_params(L=4), 64).cuda()
    data = bench.make_data(64, 1, 1, "cuda")
    with torch.no_grad():
        ref = [o.cpu().numpy() for o in model(data)["classified_edges"]]
    assert sorted(res["config"]["outputs_dumped"]) == [f"classified_edges_{i}" for i in range(3)]
    for i, want in enumerate(ref):
        got = np.load(tmp_path / f"classified_edges_{i}.npy")
        assert got.dtype == np.float32 and got.shape == (64 * 63, 1)
        assert np.array_equal(got, want), (i, float(np.abs(got - want).max()))
