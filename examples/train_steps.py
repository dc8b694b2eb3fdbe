#!/usr/bin/env python3
"""Training through the HIP path (train.py:454-494 of the reference: forward, BCE over the classified steps, backward, SGD) on
synthetic frames -- once with the shipped training configuration (fused training kernels, the whole iteration replayed as one HIP
graph) and once with BatchNorm + Dropout switched on in every MLP (the layer-by-layer engine); before them, a short leg that trains a ReID
head THROUGH the GPU graph build (build_graph_batch is differentiable with respect to the raw embeddings).  GPU box:
    python examples/train_steps.py
"""
import copy
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (graph_net_params: the reference's GRAPH_NET_PARAMS)
from gnn_cca_amd import MOTMPNet  # noqa: E402
from gnn_cca_amd.training import GraphedTrainStep  # noqa: E402


class Batch:
    pass


def frames(n_frames, cams, per, rng):
    """Disjoint union of cross-camera graphs (inference.py:209-216) with 2048-d node features and 4 edge attributes."""
    n_g = cams * per
    rows, cols = [], []
    cam = np.repeat(np.arange(cams), per)
    for f in range(n_frames):
        i, j = np.meshgrid(np.arange(n_g), np.arange(n_g), indexing="ij")
        m = cam[i] != cam[j]
        rows.append(i[m] + f * n_g), cols.append(j[m] + f * n_g)
    ei = np.stack([np.concatenate(rows), np.concatenate(cols)])
    b = Batch()
    b.x = torch.from_numpy(rng.standard_normal((n_frames * n_g, 2048)).astype(np.float32) * 0.05).cuda()
    b.edge_index = torch.from_numpy(ei).cuda()
    b.edge_attr = torch.from_numpy(rng.random((ei.shape[1], 4)).astype(np.float32)).cuda()
    labels = torch.from_numpy((rng.random(ei.shape[1]) < 0.25).astype(np.float32)).cuda()
    return b, labels


def run(title, params, steps=30):
    torch.manual_seed(0)
    model = MOTMPNet(copy.deepcopy(params), None, "resnet50").cuda().train()
    model.set_dropout_seed(1)
    opt = torch.optim.SGD(model.parameters(), lr=0.05, momentum=0.9)
    crit = torch.nn.BCEWithLogitsLoss()
    loss_fn = lambda out, lab: sum(crit(o.view(-1), lab) for o in out["classified_edges"])   # train.py:80-97
    step = GraphedTrainStep(model, opt, loss_fn, warmup=3)
    rng = np.random.default_rng(0)
    batch, labels = frames(32, 4, 6, rng)
    losses = []
    for it in range(steps):
        batch.edge_attr = torch.from_numpy(rng.random(tuple(batch.edge_attr.shape)).astype(np.float32)).cuda()
        losses.append(float(step(batch, labels)))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        step(batch, labels)
    torch.cuda.synchronize()
    print(f"{title}: engine = {model._train_path}, loss {losses[0]:.4f} -> {losses[-1]:.4f}, {(time.perf_counter() - t0) / 20 * 1e3:.2f} ms per "
          f"training step (N = {batch.x.shape[0]}, E = {batch.edge_index.shape[1]}, replayed HIP graph)")
    assert losses[-1] < losses[0]
    # inputs that require grad receive theirs: a small projection in front of the MPN (a ReID head, say) trains through the same loss
    # (both figures are zero when the ReLUs of the node path have died, which un-scaled 'sum' aggregation does to random weights)
    head = torch.nn.Linear(256, 2048).cuda()
    proj = Batch()
    proj.x, proj.edge_index, proj.edge_attr = 0.05 * head(torch.randn(batch.x.shape[0], 256, device="cuda")), batch.edge_index, batch.edge_attr
    model.zero_grad(set_to_none=True)
    loss_fn(model(proj), labels).backward()
    print(f"{title}: a projection in front of the MPN receives max|d loss / d head.weight| = {float(head.weight.grad.abs().max()):.3e} "
          f"(first encoder layer: {float(model.encoder.node_mlp.fc_layers[0].weight.grad.abs().max()):.3e})")


def head_through_graph_build(params, steps=20):
    """A ReID head trained through the association loss: nn.Linear head -> build_graph_batch (differentiable: the gradients of x and
    edge_attr reach the raw embeddings through the normalisation and the edge attributes) -> MOTMPNet.train() -> EdgeLoss -> backward ->
    an optimizer step on the head alone."""
    from gnn_cca_amd.graph_build import build_graph_batch
    from gnn_cca_amd.loss import EdgeLoss
    torch.manual_seed(0)
    rng = np.random.default_rng(1)
    model = MOTMPNet(copy.deepcopy(params), None, "resnet50").cuda().train()
    head = torch.nn.Linear(128, 2048).cuda()
    opt = torch.optim.SGD(head.parameters(), lr=0.5)
    loss_fn = EdgeLoss("BCE")
    n_frames, cams, per = 8, 4, 5
    n = n_frames * cams * per
    id_cam = np.tile(np.repeat(np.arange(cams), per), n_frames)
    ids = np.concatenate([rng.permutation(per)[np.arange(cams * per) % per] for _ in range(n_frames)])   # every person once per camera
    crops = torch.from_numpy((np.eye(per, 128)[ids] + 0.3 * rng.standard_normal((n, 128))).astype(np.float32)).cuda()   # stand-in for the CNN input
    xw, yw = rng.uniform(-10, 10, n), rng.uniform(-10, 10, n)
    losses = []
    for _ in range(steps):
        emb = head(crops)
        batch = build_graph_batch(xw, yw, ids, id_cam, [cams * per] * n_frames, [40.0] * n_frames, emb, emb)
        loss = loss_fn(model(batch), batch.edge_labels)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    print(f"ReID head through the graph build: loss {losses[0]:.4f} -> {losses[-1]:.4f} over {steps} steps on the head alone "
          f"(max|d loss / d head.weight| = {float(head.weight.grad.abs().max()):.3e})")
    assert head.weight.grad is not None and np.isfinite(losses).all()


if __name__ == "__main__":
    head_through_graph_build(bench.graph_net_params(cls_bn=False))
    run("shipped training configuration", bench.graph_net_params(cls_bn=False))
    p = bench.graph_net_params(cls_bn=True)
    p["encoder_feats_dict"]["nodes"]["resnet50"].update(use_batchnorm=True, dropout_p=0.1)
    p["edge_model_feats_dict"].update(use_batchnorm=True, dropout_p=0.1)
    p["node_model_feats_dict"].update(use_batchnorm=True, dropout_p=0.1)
    p["classifier_feats_dict"]["dropout_p"] = 0.1
    run("BatchNorm + Dropout in every MLP", p)
