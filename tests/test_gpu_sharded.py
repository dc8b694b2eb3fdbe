"""SURVEY.md 8(e) on hardware: two FRESH rank processes (RCCL when the box has two GPUs, gloo with both ranks on
cuda:0 otherwise) broadcast rank 0's weights and run sharding.forward_sharded over 7 unequal graphs; every graph's
logits must be BITWISE equal to the unsharded single-process forward over the union of all 7.  (All three launches
-- the 7-graph union and the 4- and 3-graph shares -- fall into the same dispatch regime: N < 992 keeps the encoder's
split-K factor, out-degree < 64 keeps one wave per segment; a graph's result then does not depend on its neighbours
in the batch.)  Also: `bench.py --gpus 2` with WORLD_SIZE unset starts its own rank processes and reports n_gpus 2."""
import copy
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, ROOT
from oracle.mpn_oracle import load_case

pytestmark = pytest.mark.gpu

WORKER = os.path.join(ROOT, "tests", "helpers", "sharded_worker.py")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _clean_env():
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return env


def test_forward_sharded_two_ranks_bitwise_equals_unsharded(tmp_path):
    world, port = 2, _free_port()
    procs = [subprocess.Popen([sys.executable, WORKER, str(r), str(world), str(port), str(tmp_path)], env=_clean_env())
             for r in range(world)]
    try:
        for p in procs:
            assert p.wait(timeout=300) == 0
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
    from sharded_worker import SIZES, make_graphs
    from gnn_cca_amd import MOTMPNet
    from gnn_cca_amd.sharding import split_logits, union_graphs
    params, arch, sd, _ = load_case(os.path.join(GOLDEN_DIR, "terrace32.npz"))
    m = MOTMPNet(copy.deepcopy(params), None, arch)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    m = m.cuda().eval()
    batch = union_graphs(make_graphs("cuda"))
    with torch.no_grad():
        ref = split_logits(m(batch), batch)
    torch.cuda.synchronize()
    got = [np.load(os.path.join(tmp_path, f"rank{r}.npz")) for r in range(world)]
    covered = []
    for r, z in enumerate(got):
        lo, hi = int(z["lo"]), int(z["hi"])
        covered += list(range(lo, hi))
        for k, v in sd.items():   # the broadcast put rank 0's state_dict into every rank's own tensors
            assert np.array_equal(z["sd::" + k], np.asarray(v)), (r, k)
        for g in range(lo, hi):
            assert len(ref[g]) == 3
            for s, t in enumerate(ref[g]):
                a = z[f"g{g}_s{s}"]
                assert a.shape == (SIZES[g] * (SIZES[g] - 1), 1)
                assert np.array_equal(a, t.cpu().numpy()), (r, g, s, float(np.abs(a - t.cpu().numpy()).max()))
    assert covered == list(range(len(SIZES)))
    assert str(got[0]["backend"]) == ("nccl" if torch.cuda.device_count() >= world else "gloo")


def test_bench_launches_its_own_ranks():
    """`python bench.py --gpus 2` (WORLD_SIZE unset): the parent starts two rank processes; rank 0 prints ONE JSON line
    with n_gpus = 2 and the sharded config-4 leg."""
    multi = torch.cuda.device_count() >= 2
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "5", "--warmup", "2", "--min-blocks", "3",
           "--no-cpu-baseline", "--no-scale-probe", "--profile-reps", "1", "--config4-graphs", "6", "--mode", "eager", "--full"]
    if not multi:
        cmd += ["--single-device", "--backend", "gloo"]
    r = subprocess.run(cmd, env=_clean_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    assert res["n_gpus"] == 2 and res["steps"] == 5 and res["config"]["outputs_finite"]
    assert res["value"] > 0 and res["scaling"] == "weak"
    c4 = res["config4_sharded"]
    assert c4["n_gpus"] == 2 and c4["graphs_per_rank"] == 3 and c4["outputs_finite"] and c4["value"] > 0


def test_shard_vs_union_across_dispatch_regimes_is_bounded():
    """BASELINE config 4 as the 8-GPU run sees it: a rank's 64 x dense128 share (N = 8192: split-K encoder GEMM + MFMA tail, one
    node per wave) against the SAME 64 graphs inside the 512-graph union on one GPU (N = 65 536: un-split GEMM with the fused
    epilogue, persistent step waves).  The step kernels are the same arithmetic in both regimes; the first encoder layer sums its
    2048 products in another order (split-K slabs), so a graph's logits are NOT bitwise independent of how many graphs share its
    forward -- they agree within rounding, and this test states the bound: <= 2e-6 on O(0.5) logits.  (Inside one regime the
    result is bitwise independent of the batch neighbours: test_forward_sharded_two_ranks_bitwise_equals_unsharded.)"""
    import bench
    from gnn_cca_amd.sharding import shard_range
    g_all, n, world = 512, 128, 8
    model = bench.build_model(bench.graph_net_params(), n).cuda()
    dev = torch.device("cuda", 0)
    union = bench.make_data(n, g_all, 5, dev)
    e_per = n * (n - 1)
    with torch.no_grad():
        full = [t.clone() for t in model(union)["classified_edges"]]
    worst = 0.0
    for rank in (0, 5):    # two of the eight shares
        lo, hi = shard_range(g_all, rank, world)
        assert hi - lo == 64
        share = bench.Data()
        share.x = union.x[lo * n:hi * n].contiguous()
        share.edge_index = (union.edge_index[:, lo * e_per:hi * e_per] - lo * n).contiguous()
        share.edge_attr = union.edge_attr[lo * e_per:hi * e_per].contiguous()
        with torch.no_grad():
            part = model(share)["classified_edges"]
        for a, b in zip(part, full):
            ref = b[lo * e_per:hi * e_per]
            assert torch.isfinite(a).all()
            worst = max(worst, float((a - ref).abs().max()))
        # run to run, and between the two shares' own forwards, everything is deterministic
        with torch.no_grad():
            again = model(share)["classified_edges"]
        assert all(torch.equal(x, y) for x, y in zip(part, again))
    assert worst <= 2e-6, worst
    print(f"shard (64 of 512 x dense128) vs union: max |dlogit| = {worst:.3e}")


def test_unsplit_encoder_option_makes_shards_bitwise_equal_to_the_union():
    """`model.encoder_unsplit = True` (GNNCCA_OPT_ENC_UNSPLIT): forwards over >= 4096 nodes never split K in the first encoder
    layer -- the 32-row un-split kernel (shares of 8192 / 16 384 / 4096 + nodes) and the 256-row un-split kernel (the 65 536-node
    union) run the same per-element arithmetic, so a graph's logits are BIT FOR BIT what the union computes: the 8-, 4- and 16-rank
    shares of BASELINE config 4 against the 512-graph union on one GPU."""
    import bench
    from gnn_cca_amd.sharding import shard_range
    g_all, n = 512, 128
    model = bench.build_model(bench.graph_net_params(), n).cuda()
    model.encoder_unsplit = True
    dev = torch.device("cuda", 0)
    union = bench.make_data(n, g_all, 5, dev)
    e_per = n * (n - 1)
    with torch.no_grad():
        full = [t.clone() for t in model(union)["classified_edges"]]
    for world, rank in ((8, 0), (8, 5), (4, 3), (16, 9)):
        lo, hi = shard_range(g_all, rank, world)
        share = bench.Data()
        share.x = union.x[lo * n:hi * n].contiguous()
        share.edge_index = (union.edge_index[:, lo * e_per:hi * e_per] - lo * n).contiguous()
        share.edge_attr = union.edge_attr[lo * e_per:hi * e_per].contiguous()
        with torch.no_grad():
            part = model(share)["classified_edges"]
        for a, b in zip(part, full):
            assert torch.equal(a, b[lo * e_per:hi * e_per]), (world, rank, float((a - b[lo * e_per:hi * e_per]).abs().max()))


def test_unsplit_option_with_long_segments_shard_of_two_dense2048_equals_union_of_eight():
    """waves-per-node is a function of the batch's node count for graphs whose nodes average >= 32 chunks
    (degree ~2000+) -- a shard of 2 x dense2048 (N = 4096) would run four waves per node, the union of 8 (N = 16 384) one, and the
    cross-wave combine sums in another order.  With GNNCCA_OPT_ENC_UNSPLIT the forward pins one wave per node from 4096 nodes on, so
    the documented guarantee (batch-independent logits for batches of >= 4096 nodes) holds for long segments too: bitwise."""
    import bench
    n, g_all = 2048, 8
    model = bench.build_model(bench.graph_net_params(), n).cuda()
    model.encoder_unsplit = True
    dev = torch.device("cuda", 0)
    union = bench.make_data(n, g_all, 11, dev)
    e_per = n * (n - 1)
    with torch.no_grad():
        full = [t.clone() for t in model(union)["classified_edges"]]
        assert all(torch.isfinite(t).all() for t in full)
        for lo, hi in ((0, 2), (4, 6), (5, 8)):
            share = bench.Data()
            share.x = union.x[lo * n:hi * n].contiguous()
            share.edge_index = (union.edge_index[:, lo * e_per:hi * e_per] - lo * n).contiguous()
            share.edge_attr = union.edge_attr[lo * e_per:hi * e_per].contiguous()
            part = model(share)["classified_edges"]
            for a, b in zip(part, full):
                assert torch.equal(a, b[lo * e_per:hi * e_per]), (lo, hi, float((a - b[lo * e_per:hi * e_per]).abs().max()))
            del share, part


def test_unsplit_option_bitwise_shares_hold_for_the_documented_encoder_shapes():
    """include/gnncca_mpn.h states which encoders GNNCCA_OPT_ENC_UNSPLIT makes batch-independent: two layers, the first 128 wide,
    node_in_dim a multiple of 256, no reattach_initial_nodes -- not only the shipped 2048 -> 128 -> 32.  Here node_in_dim 512: shares
    of 4096, 6144 and 10 240 nodes (the 32-row un-split kernel) against the 65 536-node union (the 256-row un-split kernel, one round
    of workgroups), every logit bit for bit.  Sparse ring graphs of 256 nodes, random weights."""
    from gnn_cca_amd import MOTMPNet
    import bench
    params = copy.deepcopy(bench.graph_net_params())
    params["encoder_feats_dict"]["nodes"]["resnet50"]["node_in_dim"] = 512
    torch.manual_seed(21)
    model = MOTMPNet(params, None, "resnet50")
    with torch.no_grad():
        for p in model.MPNet.node_model.node_mlp.parameters():
            p.mul_(1.0 / 3)
    model = model.cuda().eval()
    model.encoder_unsplit = True
    n, g_all, hops = 256, 256, (1, 5, 17)
    rng = np.random.default_rng(21)
    x = torch.from_numpy(rng.standard_normal((n * g_all, 512)).astype(np.float32)).cuda()
    src = np.repeat(np.arange(n), len(hops))
    one = np.stack([src, (src + np.tile(list(hops), n)) % n])
    e_per = one.shape[1]
    ei = torch.from_numpy(np.concatenate([one + g * n for g in range(g_all)], axis=1).astype(np.int64)).cuda()
    ea = torch.from_numpy(rng.random((ei.shape[1], 4)).astype(np.float32)).cuda()
    union = bench.Data()
    union.x, union.edge_index, union.edge_attr = x, ei, ea
    with torch.no_grad():
        full = [t.clone() for t in model(union)["classified_edges"]]
    assert all(torch.isfinite(t).all() for t in full)
    for lo, hi in ((0, 16), (100, 124), (216, 256)):
        share = bench.Data()
        share.x = x[lo * n:hi * n].contiguous()
        share.edge_index = (ei[:, lo * e_per:hi * e_per] - lo * n).contiguous()
        share.edge_attr = ea[lo * e_per:hi * e_per].contiguous()
        with torch.no_grad():
            part = model(share)["classified_edges"]
        for a, b in zip(part, full):
            assert torch.equal(a, b[lo * e_per:hi * e_per]), (lo, hi, float((a - b[lo * e_per:hi * e_per]).abs().max()))
