"""The message steps' route table (csrc/step_route.cpp: step_plan, step_launch), pinned on the CPU.

step_plan() decides once per forward what does not change from step to step -- the kernel family, the message arithmetic, waves per
node, nodes per wave, the LDS gather table, the cache policy, column ranges, the padded layout, deferred classification -- and
step_launch() names, per step, exactly one kernel instantiation with its grid, its dynamic LDS and the logit slots it writes;
launch_step_variant (csrc/mpn_forward.hip) carries that out and compares no sizes.  Here a stand-alone host program (plain C++ against
internal.h, pack.cpp and step_route.cpp: no HIP, no GPU) prints the route of every case with the default StepTuning, or with ONE field
of it overridden, and the test holds the output against the table below -- written from the conditions of the forward as it was before
the route became a function (that dispatch code, run on the host with its launches replaced by prints: DESIGN.md 4.2).  A pull request
that adds a variant or moves a threshold edits this table on purpose.

A line reads: fam = family, f32 = StepParams::msg_f32, vec = attr_vec, wps = waves per node, npw = nodes per wave of step 1 / of the
later steps, pdl = LDS gather table, eb = bf16 edge state, nt = cache policy, rng = column ranges, ell = padded layout's slots per node as
used, defer = deferred classification, fc = first classifying step; then per step the instantiation -- GEN<RE,MSG,MX>,
FAST<FIRST,CLS,MSG,PDL,EB,NT> or PIPE<FIRST,CLS,MSG,PDL,EB,NT,RNG,NPW,CIN> --, g = workgroups, lds = dynamic LDS bytes, out / in = the
logit slot written / classified from the input state (-1: none).  The graphs have `deg` edges per node (3 unless given), the shipped dims,
L = 4 steps of which 2 classify, aligned inputs and no trace unless stated."""
import os
import re
import subprocess

import pytest

from conftest import ROOT
from test_workspace_layouts import _host_compiler

CSRC = os.path.join(ROOT, "gnn-cca_amd", "csrc")
FLAGS = {"traced": 1, "trace_h": 2, "agg_max": 4, "edge_in5": 8, "reattach_edges": 16, "reattach_nodes": 32, "unaligned": 64, "dropping": 128,
         "unsplit": 256, "bf16": 512, "ranges": 1024}


def C(n, deg=3, E=None, L=4, cls=2, tune=None, **flags):
    """One case as the probe's argument: N:E:L:class steps:flag bits[:StepTuning field=value]."""
    bits = sum(FLAGS[k] for k, v in flags.items() if v)
    return f"{n}:{n * deg if E is None else E}:{L}:{cls}:{bits}" + (f":{tune[0]}={tune[1]}" if tune else "")


TABLE = [
    # family
    (C(64, E=4032),
     "fam=FAST f32=1 vec=1 wps=1 npw=1/1 pdl=0 eb=0 nt=0 rng=0 ell=0 defer=0 fc=3 L=4 | FAST<1,0,1,0,0,0> g=16 lds=6720 out=-1 in=-1 | FAST<0,0,1,0,0,0> g=16 lds=6720 out=-1 in=-1 | FAST<0,1,1,0,0,0> g=16 lds=6720 out=0 in=-1 | FAST<0,1,0,0,0,0> g=16 lds=576 out=1 in=-1"),
    (C(512),
     "fam=FAST f32=1 vec=1 wps=1 npw=1/1 pdl=0 eb=0 nt=0 rng=0 ell=0 defer=0 fc=3 L=4 | FAST<1,0,1,0,0,0> g=128 lds=6720 out=-1 in=-1 | FAST<0,0,1,0,0,0> g=128 lds=6720 out=-1 in=-1 | FAST<0,1,1,0,0,0> g=128 lds=6720 out=0 in=-1 | FAST<0,1,0,0,0,0> g=128 lds=576 out=1 in=-1"),
    (C(513),
     "fam=PIPE f32=0 vec=1 wps=1 npw=1/1 pdl=0 eb=0 nt=0 rng=0 ell=0 defer=0 fc=3 L=4 | PIPE<1,0,1,0,0,0,0,1,0> g=129 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,1,0> g=129 lds=6720 out=-1 in=-1 | PIPE<0,1,1,0,0,0,0,1,0> g=129 lds=6720 out=0 in=-1 | PIPE<0,1,0,0,0,0,0,1,0> g=129 lds=576 out=1 in=-1"),
    (C(513, traced=True),
     "fam=GEN f32=0 vec=1 wps=1 npw=1/1 pdl=0 eb=0 nt=0 rng=0 ell=0 defer=0 fc=3 L=4 | GEN<0,1,0> g=129 lds=6656 out=-1 in=-1 | GEN<0,1,0> g=129 lds=6656 out=-1 in=-1 | GEN<0,1,0> g=129 lds=6656 out=0 in=-1 | GEN<0,0,0> g=129 lds=512 out=1 in=-1"),
    (C(513, traced=True, trace_h=True),
     "fam=GEN f32=0 vec=1 wps=1 npw=1/1 pdl=0 eb=0 nt=0 rng=0 ell=0 defer=0 fc=3 L=4 | GEN<0,1,0> g=129 lds=6656 out=-1 in=-1 | GEN<0,1,0> g=129 lds=6656 out=-1 in=-1 | GEN<0,1,0> g=129 lds=6656 out=0 in=-1 | GEN<0,1,0> g=129 lds=6656 out=1 in=-1"),
    (C(513, traced=True, trace_h=True, dropping=True),
     "fam=GEN f32=0 vec=1 wps=1 npw=1/1 pdl=0 eb=0 nt=0 rng=0 ell=0 defer=0 fc=3 L=4 | GEN<0,1,0> g=129 lds=6656 out=-1 in=-1 | GEN<0,1,0> g=129 lds=6656 out=-1 in=-1 | GEN<0,1,0> g=129 lds=6656 out=0 in=-1 | GEN<0,1,0> g=129 lds=6656 out=1 in=-1"),
    (C(513, agg_max=True),
     "fam=GEN f32=0 vec=1 wps=1 npw=1/1 pdl=0 eb=0 nt=0 rng=0 ell=0 defer=0 fc=3 L=4 | GEN<0,1,1> g=129 lds=6656 out=-1 in=-1 | GEN<0,1,1> g=129 lds=6656 out=-1 in=-1 | GEN<0,1,1> g=129 lds=6656 out=0 in=-1 | GEN<0,0,1> g=129 lds=512 out=1 in=-1"),
    (C(513, edge_in5=True),
     "fam=GEN f32=0 vec=0 wps=1 npw=1/1 pdl=0 eb=0 nt=0 rng=0 ell=0 defer=0 fc=3 L=4 | GEN<0,1,0> g=129 lds=6656 out=-1 in=-1 | GEN<0,1,0> g=129 lds=6656 out=-1 in=-1 | GEN<0,1,0> g=129 lds=6656 out=0 in=-1 | GEN<0,0,0> g=129 lds=512 out=1 in=-1"),
    (C(513, reattach_edges=True),
     "fam=GEN f32=0 vec=1 wps=1 npw=1/1 pdl=0 eb=0 nt=0 rng=0 ell=0 defer=0 fc=3 L=4 | GEN<1,1,0> g=129 lds=6656 out=-1 in=-1 | GEN<1,1,0> g=129 lds=6656 out=-1 in=-1 | GEN<1,1,0> g=129 lds=6656 out=0 in=-1 | GEN<1,0,0> g=129 lds=512 out=1 in=-1"),
    (C(513, reattach_edges=True, agg_max=True),
     "fam=GEN f32=0 vec=1 wps=1 npw=1/1 pdl=0 eb=0 nt=0 rng=0 ell=0 defer=0 fc=3 L=4 | GEN<1,1,1> g=129 lds=6656 out=-1 in=-1 | GEN<1,1,1> g=129 lds=6656 out=-1 in=-1 | GEN<1,1,1> g=129 lds=6656 out=0 in=-1 | GEN<1,0,1> g=129 lds=512 out=1 in=-1"),
    (C(513, reattach_nodes=True),
     "fam=GEN f32=0 vec=1 wps=1 npw=1/1 pdl=0 eb=0 nt=0 rng=0 ell=0 defer=0 fc=3 L=4 | GEN<0,1,0> g=129 lds=12800 out=-1 in=-1 | GEN<0,1,0> g=129 lds=12800 out=-1 in=-1 | GEN<0,1,0> g=129 lds=12800 out=0 in=-1 | GEN<0,0,0> g=129 lds=512 out=1 in=-1"),
    (C(513, unaligned=True),
     "fam=GEN f32=0 vec=0 wps=1 npw=1/1 pdl=0 eb=0 nt=0 rng=0 ell=0 defer=0 fc=3 L=4 | GEN<0,1,0> g=129 lds=6656 out=-1 in=-1 | GEN<0,1,0> g=129 lds=6656 out=-1 in=-1 | GEN<0,1,0> g=129 lds=6656 out=0 in=-1 | GEN<0,0,0> g=129 lds=512 out=1 in=-1"),
    (C(716800, E=91033600, cls=3),
     "fam=FAST f32=1 vec=1 wps=1 npw=2/2 pdl=0 eb=0 nt=2 rng=0 ell=128 defer=0 fc=2 L=4 | FAST<1,0,1,0,0,2> g=179200 lds=6720 out=-1 in=-1 | FAST<0,1,1,0,0,2> g=179200 lds=6720 out=0 in=-1 | FAST<0,1,1,0,0,2> g=179200 lds=6720 out=1 in=-1 | FAST<0,1,0,0,0,2> g=179200 lds=576 out=2 in=-1"),
    # waves per node
    (C(600, deg=64),
     "fam=PIPE f32=0 vec=1 wps=1 npw=1/1 pdl=0 eb=0 nt=0 rng=0 ell=0 defer=0 fc=3 L=4 | PIPE<1,0,1,0,0,0,0,1,0> g=150 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,1,0> g=150 lds=6720 out=-1 in=-1 | PIPE<0,1,1,0,0,0,0,1,0> g=150 lds=6720 out=0 in=-1 | PIPE<0,1,0,0,0,0,0,1,0> g=150 lds=576 out=1 in=-1"),
    (C(600, deg=65),
     "fam=PIPE f32=0 vec=1 wps=2 npw=1/1 pdl=0 eb=0 nt=0 rng=0 ell=0 defer=0 fc=3 L=4 | PIPE<1,0,1,0,0,0,0,1,0> g=300 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,1,0> g=300 lds=6720 out=-1 in=-1 | PIPE<0,1,1,0,0,0,0,1,0> g=300 lds=6720 out=0 in=-1 | PIPE<0,1,0,0,0,0,0,1,0> g=300 lds=576 out=1 in=-1"),
    (C(600, deg=192),
     "fam=PIPE f32=0 vec=1 wps=2 npw=1/1 pdl=0 eb=0 nt=0 rng=0 ell=0 defer=0 fc=3 L=4 | PIPE<1,0,1,0,0,0,0,1,0> g=300 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,1,0> g=300 lds=6720 out=-1 in=-1 | PIPE<0,1,1,0,0,0,0,1,0> g=300 lds=6720 out=0 in=-1 | PIPE<0,1,0,0,0,0,0,1,0> g=300 lds=576 out=1 in=-1"),
    (C(600, deg=193),
     "fam=PIPE f32=0 vec=1 wps=4 npw=1/1 pdl=0 eb=0 nt=0 rng=0 ell=0 defer=0 fc=3 L=4 | PIPE<1,0,1,0,0,0,0,1,0> g=600 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,1,0> g=600 lds=6720 out=-1 in=-1 | PIPE<0,1,1,0,0,0,0,1,0> g=600 lds=6720 out=0 in=-1 | PIPE<0,1,0,0,0,0,0,1,0> g=600 lds=576 out=1 in=-1"),
    (C(2048, deg=260),
     "fam=PIPE f32=0 vec=1 wps=2 npw=1/1 pdl=0 eb=0 nt=0 rng=0 ell=288 defer=0 fc=3 L=4 | PIPE<1,0,1,0,0,0,0,1,0> g=1024 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,1,0> g=1024 lds=6720 out=-1 in=-1 | PIPE<0,1,1,0,0,0,0,1,0> g=1024 lds=6720 out=0 in=-1 | PIPE<0,1,0,0,0,0,0,1,0> g=1024 lds=576 out=1 in=-1"),
    (C(4097, deg=260),
     "fam=PIPE f32=0 vec=1 wps=1 npw=1/1 pdl=0 eb=0 nt=0 rng=0 ell=288 defer=0 fc=3 L=4 | PIPE<1,0,1,0,0,0,0,1,0> g=1025 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,1,0> g=1025 lds=6720 out=-1 in=-1 | PIPE<0,1,1,0,0,0,0,1,0> g=1025 lds=6720 out=0 in=-1 | PIPE<0,1,0,0,0,0,0,1,0> g=1025 lds=576 out=1 in=-1"),
    (C(2100, E=2100 * 2099),
     "fam=PIPE f32=0 vec=1 wps=4 npw=1/1 pdl=0 eb=0 nt=0 rng=0 ell=2112 defer=0 fc=3 L=4 | PIPE<1,0,1,0,0,0,0,1,0> g=2100 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,1,0> g=2100 lds=6720 out=-1 in=-1 | PIPE<0,1,1,0,0,0,0,1,0> g=2100 lds=6720 out=0 in=-1 | PIPE<0,1,0,0,0,0,0,1,0> g=2100 lds=576 out=1 in=-1"),
    (C(4095, deg=260, unsplit=True),
     "fam=PIPE f32=0 vec=1 wps=1 npw=1/1 pdl=0 eb=0 nt=0 rng=0 ell=288 defer=0 fc=3 L=4 | PIPE<1,0,1,0,0,0,0,1,0> g=1024 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,1,0> g=1024 lds=6720 out=-1 in=-1 | PIPE<0,1,1,0,0,0,0,1,0> g=1024 lds=6720 out=0 in=-1 | PIPE<0,1,0,0,0,0,0,1,0> g=1024 lds=576 out=1 in=-1"),
    (C(4096, deg=260, unsplit=True),
     "fam=PIPE f32=0 vec=1 wps=1 npw=1/1 pdl=0 eb=0 nt=0 rng=0 ell=288 defer=0 fc=3 L=4 | PIPE<1,0,1,0,0,0,0,1,0> g=1024 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,1,0> g=1024 lds=6720 out=-1 in=-1 | PIPE<0,1,1,0,0,0,0,1,0> g=1024 lds=6720 out=0 in=-1 | PIPE<0,1,0,0,0,0,0,1,0> g=1024 lds=576 out=1 in=-1"),
    (C(600, deg=260, tune=("force_wps", 1)),
     "fam=PIPE f32=0 vec=1 wps=1 npw=1/1 pdl=0 eb=0 nt=0 rng=0 ell=0 defer=0 fc=3 L=4 | PIPE<1,0,1,0,0,0,0,1,0> g=150 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,1,0> g=150 lds=6720 out=-1 in=-1 | PIPE<0,1,1,0,0,0,0,1,0> g=150 lds=6720 out=0 in=-1 | PIPE<0,1,0,0,0,0,0,1,0> g=150 lds=576 out=1 in=-1"),
    (C(600, deg=260, tune=("force_wps", 2)),
     "fam=PIPE f32=0 vec=1 wps=2 npw=1/1 pdl=0 eb=0 nt=0 rng=0 ell=0 defer=0 fc=3 L=4 | PIPE<1,0,1,0,0,0,0,1,0> g=300 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,1,0> g=300 lds=6720 out=-1 in=-1 | PIPE<0,1,1,0,0,0,0,1,0> g=300 lds=6720 out=0 in=-1 | PIPE<0,1,0,0,0,0,0,1,0> g=300 lds=576 out=1 in=-1"),
    (C(600, deg=260, tune=("force_wps", 4)),
     "fam=PIPE f32=0 vec=1 wps=4 npw=1/1 pdl=0 eb=0 nt=0 rng=0 ell=0 defer=0 fc=3 L=4 | PIPE<1,0,1,0,0,0,0,1,0> g=600 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,1,0> g=600 lds=6720 out=-1 in=-1 | PIPE<0,1,1,0,0,0,0,1,0> g=600 lds=6720 out=0 in=-1 | PIPE<0,1,0,0,0,0,0,1,0> g=600 lds=576 out=1 in=-1"),
    (C(600, deg=65, tune=("force_wps", 1)),
     "fam=PIPE f32=0 vec=1 wps=1 npw=1/1 pdl=0 eb=0 nt=0 rng=0 ell=0 defer=0 fc=3 L=4 | PIPE<1,0,1,0,0,0,0,1,0> g=150 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,1,0> g=150 lds=6720 out=-1 in=-1 | PIPE<0,1,1,0,0,0,0,1,0> g=150 lds=6720 out=0 in=-1 | PIPE<0,1,0,0,0,0,0,1,0> g=150 lds=576 out=1 in=-1"),
    (C(600, deg=65, tune=("force_wps", 2)),
     "fam=PIPE f32=0 vec=1 wps=2 npw=1/1 pdl=0 eb=0 nt=0 rng=0 ell=0 defer=0 fc=3 L=4 | PIPE<1,0,1,0,0,0,0,1,0> g=300 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,1,0> g=300 lds=6720 out=-1 in=-1 | PIPE<0,1,1,0,0,0,0,1,0> g=300 lds=6720 out=0 in=-1 | PIPE<0,1,0,0,0,0,0,1,0> g=300 lds=576 out=1 in=-1"),
    (C(600, deg=65, tune=("force_wps", 4)),
     "fam=PIPE f32=0 vec=1 wps=2 npw=1/1 pdl=0 eb=0 nt=0 rng=0 ell=0 defer=0 fc=3 L=4 | PIPE<1,0,1,0,0,0,0,1,0> g=300 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,1,0> g=300 lds=6720 out=-1 in=-1 | PIPE<0,1,1,0,0,0,0,1,0> g=300 lds=6720 out=0 in=-1 | PIPE<0,1,0,0,0,0,0,1,0> g=300 lds=576 out=1 in=-1"),
    # two nodes per wave, deferral
    (C(16383),
     "fam=PIPE f32=0 vec=1 wps=1 npw=1/1 pdl=0 eb=0 nt=0 rng=0 ell=0 defer=0 fc=3 L=4 | PIPE<1,0,1,0,0,0,0,1,0> g=4096 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,1,0> g=4096 lds=6720 out=-1 in=-1 | PIPE<0,1,1,0,0,0,0,1,0> g=4096 lds=6720 out=0 in=-1 | PIPE<0,1,0,0,0,0,0,1,0> g=4096 lds=576 out=1 in=-1"),
    (C(16384),
     "fam=PIPE f32=0 vec=1 wps=1 npw=2/2 pdl=0 eb=0 nt=0 rng=0 ell=0 defer=1 fc=3 L=4 | PIPE<1,0,1,0,0,0,0,2,0> g=2048 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,2,0> g=2048 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,2,0> g=2048 lds=6720 out=-1 in=-1 | PIPE<0,1,0,0,0,0,0,1,1> g=4096 lds=576 out=1 in=0"),
    (C(16384, cls=1),
     "fam=PIPE f32=0 vec=1 wps=1 npw=2/2 pdl=0 eb=0 nt=0 rng=0 ell=0 defer=0 fc=4 L=4 | PIPE<1,0,1,0,0,0,0,2,0> g=2048 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,2,0> g=2048 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,2,0> g=2048 lds=6720 out=-1 in=-1 | PIPE<0,1,0,0,0,0,0,1,0> g=4096 lds=576 out=0 in=-1"),
    (C(16384, cls=3),
     "fam=PIPE f32=0 vec=1 wps=1 npw=2/2 pdl=0 eb=0 nt=0 rng=0 ell=0 defer=1 fc=2 L=4 | PIPE<1,0,1,0,0,0,0,2,0> g=2048 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,2,0> g=2048 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,2,1> g=2048 lds=6720 out=-1 in=0 | PIPE<0,1,0,0,0,0,0,1,1> g=4096 lds=576 out=2 in=1"),
    (C(16384, deg=129),
     "fam=PIPE f32=0 vec=1 wps=1 npw=1/1 pdl=0 eb=0 nt=0 rng=0 ell=0 defer=0 fc=3 L=4 | PIPE<1,0,1,0,0,0,0,1,0> g=4096 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,1,0> g=4096 lds=6720 out=-1 in=-1 | PIPE<0,1,1,0,0,0,0,1,0> g=4096 lds=6720 out=0 in=-1 | PIPE<0,1,0,0,0,0,0,1,0> g=4096 lds=576 out=1 in=-1"),
    (C(8192, tune=("force_npw", 1)),
     "fam=PIPE f32=0 vec=1 wps=1 npw=1/1 pdl=0 eb=0 nt=0 rng=0 ell=0 defer=0 fc=3 L=4 | PIPE<1,0,1,0,0,0,0,1,0> g=2048 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,1,0> g=2048 lds=6720 out=-1 in=-1 | PIPE<0,1,1,0,0,0,0,1,0> g=2048 lds=6720 out=0 in=-1 | PIPE<0,1,0,0,0,0,0,1,0> g=2048 lds=576 out=1 in=-1"),
    (C(8192, tune=("force_npw", 2)),
     "fam=PIPE f32=0 vec=1 wps=1 npw=2/2 pdl=0 eb=0 nt=0 rng=0 ell=0 defer=1 fc=3 L=4 | PIPE<1,0,1,0,0,0,0,2,0> g=1024 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,2,0> g=1024 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,2,0> g=1024 lds=6720 out=-1 in=-1 | PIPE<0,1,0,0,0,0,0,1,1> g=2048 lds=576 out=1 in=0"),
    (C(16384, tune=("force_npw", 1)),
     "fam=PIPE f32=0 vec=1 wps=1 npw=1/1 pdl=0 eb=0 nt=0 rng=0 ell=0 defer=0 fc=3 L=4 | PIPE<1,0,1,0,0,0,0,1,0> g=4096 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,1,0> g=4096 lds=6720 out=-1 in=-1 | PIPE<0,1,1,0,0,0,0,1,0> g=4096 lds=6720 out=0 in=-1 | PIPE<0,1,0,0,0,0,0,1,0> g=4096 lds=576 out=1 in=-1"),
    (C(16384, tune=("npw_min_n_first", 20000)),
     "fam=PIPE f32=0 vec=1 wps=1 npw=1/2 pdl=0 eb=0 nt=0 rng=0 ell=0 defer=1 fc=3 L=4 | PIPE<1,0,1,0,0,0,0,1,0> g=4096 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,2,0> g=2048 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,2,0> g=2048 lds=6720 out=-1 in=-1 | PIPE<0,1,0,0,0,0,0,1,1> g=4096 lds=576 out=1 in=0"),
    (C(16384, bf16=True),
     "fam=PIPE f32=0 vec=1 wps=1 npw=2/2 pdl=0 eb=1 nt=0 rng=0 ell=0 defer=0 fc=3 L=4 | PIPE<1,0,1,0,1,0,0,2,0> g=2048 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,1,0,0,2,0> g=2048 lds=6720 out=-1 in=-1 | PIPE<0,1,1,0,1,0,0,1,0> g=4096 lds=6720 out=0 in=-1 | PIPE<0,1,0,0,1,0,0,1,0> g=4096 lds=576 out=1 in=-1"),
    (C(16384, ranges=True),
     "fam=PIPE f32=0 vec=1 wps=1 npw=2/2 pdl=0 eb=0 nt=0 rng=1 ell=0 defer=0 fc=3 L=4 | PIPE<1,0,1,0,0,0,1,1,0> g=4096 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,1,1,0> g=4096 lds=6720 out=-1 in=-1 | PIPE<0,1,1,0,0,0,1,1,0> g=4096 lds=6720 out=0 in=-1 | PIPE<0,1,0,0,0,0,1,1,0> g=4096 lds=576 out=1 in=-1"),
    # ranges
    (C(64, E=4032, ranges=True),
     "fam=FAST f32=1 vec=1 wps=1 npw=1/1 pdl=0 eb=0 nt=0 rng=1 ell=0 defer=0 fc=3 L=4 | FAST<1,0,1,0,0,0> g=16 lds=6720 out=-1 in=-1 | FAST<0,0,1,0,0,0> g=16 lds=6720 out=-1 in=-1 | FAST<0,1,1,0,0,0> g=16 lds=6720 out=0 in=-1 | FAST<0,1,0,0,0,0> g=16 lds=576 out=1 in=-1"),
    (C(513, ranges=True),
     "fam=PIPE f32=0 vec=1 wps=1 npw=1/1 pdl=0 eb=0 nt=0 rng=1 ell=0 defer=0 fc=3 L=4 | PIPE<1,0,1,0,0,0,1,1,0> g=129 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,1,1,0> g=129 lds=6720 out=-1 in=-1 | PIPE<0,1,1,0,0,0,1,1,0> g=129 lds=6720 out=0 in=-1 | PIPE<0,1,0,0,0,0,1,1,0> g=129 lds=576 out=1 in=-1"),
    (C(513, L=1, cls=1, ranges=True),
     "fam=PIPE f32=0 vec=1 wps=1 npw=1/1 pdl=0 eb=0 nt=0 rng=0 ell=0 defer=0 fc=1 L=1 | PIPE<1,1,0,0,0,0,0,1,0> g=129 lds=576 out=0 in=-1"),
    (C(513, ranges=True, tune=("force_nt", 1)),
     "fam=PIPE f32=0 vec=1 wps=1 npw=1/1 pdl=0 eb=0 nt=1 rng=1 ell=0 defer=0 fc=3 L=4 | PIPE<1,0,1,0,0,1,0,1,0> g=129 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,1,0,1,0> g=129 lds=6720 out=-1 in=-1 | PIPE<0,1,1,0,0,1,0,1,0> g=129 lds=6720 out=0 in=-1 | PIPE<0,1,0,0,0,1,0,1,0> g=129 lds=576 out=1 in=-1"),
    (C(513, ranges=True, tune=("pd_lds_min", 1)),
     "fam=PIPE f32=0 vec=1 wps=1 npw=1/1 pdl=1 eb=0 nt=0 rng=1 ell=0 defer=0 fc=3 L=4 | PIPE<1,0,1,1,0,0,1,1,0> g=129 lds=23168 out=-1 in=-1 | PIPE<0,0,1,1,0,0,1,1,0> g=129 lds=23168 out=-1 in=-1 | PIPE<0,1,1,1,0,0,1,1,0> g=129 lds=23168 out=0 in=-1 | PIPE<0,1,0,1,0,0,1,1,0> g=129 lds=17024 out=1 in=-1"),
    # cache policy
    (C(513, tune=("force_nt", 0)),
     "fam=PIPE f32=0 vec=1 wps=1 npw=1/1 pdl=0 eb=0 nt=0 rng=0 ell=0 defer=0 fc=3 L=4 | PIPE<1,0,1,0,0,0,0,1,0> g=129 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,1,0> g=129 lds=6720 out=-1 in=-1 | PIPE<0,1,1,0,0,0,0,1,0> g=129 lds=6720 out=0 in=-1 | PIPE<0,1,0,0,0,0,0,1,0> g=129 lds=576 out=1 in=-1"),
    (C(513, tune=("force_nt", 1)),
     "fam=PIPE f32=0 vec=1 wps=1 npw=1/1 pdl=0 eb=0 nt=1 rng=0 ell=0 defer=0 fc=3 L=4 | PIPE<1,0,1,0,0,1,0,1,0> g=129 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,1,0,1,0> g=129 lds=6720 out=-1 in=-1 | PIPE<0,1,1,0,0,1,0,1,0> g=129 lds=6720 out=0 in=-1 | PIPE<0,1,0,0,0,1,0,1,0> g=129 lds=576 out=1 in=-1"),
    (C(513, tune=("force_nt", 2)),
     "fam=PIPE f32=0 vec=1 wps=1 npw=1/1 pdl=0 eb=0 nt=2 rng=0 ell=0 defer=0 fc=3 L=4 | PIPE<1,0,1,0,0,2,0,1,0> g=129 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,2,0,1,0> g=129 lds=6720 out=-1 in=-1 | PIPE<0,1,1,0,0,2,0,1,0> g=129 lds=6720 out=0 in=-1 | PIPE<0,1,0,0,0,2,0,1,0> g=129 lds=576 out=1 in=-1"),
    (C(64, E=4032, tune=("force_nt", 2)),
     "fam=FAST f32=1 vec=1 wps=1 npw=1/1 pdl=0 eb=0 nt=2 rng=0 ell=0 defer=0 fc=3 L=4 | FAST<1,0,1,0,0,2> g=16 lds=6720 out=-1 in=-1 | FAST<0,0,1,0,0,2> g=16 lds=6720 out=-1 in=-1 | FAST<0,1,1,0,0,2> g=16 lds=6720 out=0 in=-1 | FAST<0,1,0,0,0,2> g=16 lds=576 out=1 in=-1"),
    (C(160000, E=6249984),
     "fam=PIPE f32=0 vec=1 wps=1 npw=2/2 pdl=0 eb=0 nt=0 rng=0 ell=0 defer=1 fc=3 L=4 | PIPE<1,0,1,0,0,0,0,2,0> g=20000 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,2,0> g=20000 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,2,0> g=20000 lds=6720 out=-1 in=-1 | PIPE<0,1,0,0,0,0,0,1,1> g=40000 lds=576 out=1 in=0"),
    (C(160000, E=6249985),
     "fam=PIPE f32=0 vec=1 wps=1 npw=2/2 pdl=0 eb=0 nt=1 rng=0 ell=0 defer=1 fc=3 L=4 | PIPE<1,0,1,0,0,1,0,2,0> g=20000 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,1,0,2,0> g=20000 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,1,0,2,0> g=20000 lds=6720 out=-1 in=-1 | PIPE<0,1,0,0,0,1,0,1,1> g=40000 lds=576 out=1 in=0"),
    (C(160000, E=10666624),
     "fam=PIPE f32=0 vec=1 wps=1 npw=2/2 pdl=0 eb=0 nt=1 rng=0 ell=0 defer=1 fc=3 L=4 | PIPE<1,0,1,0,0,1,0,2,0> g=20000 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,1,0,2,0> g=20000 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,1,0,2,0> g=20000 lds=6720 out=-1 in=-1 | PIPE<0,1,0,0,0,1,0,1,1> g=40000 lds=576 out=1 in=0"),
    (C(160000, E=10666625),
     "fam=PIPE f32=0 vec=1 wps=1 npw=2/2 pdl=0 eb=0 nt=2 rng=0 ell=0 defer=1 fc=3 L=4 | PIPE<1,0,1,0,0,2,0,2,0> g=20000 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,2,0,2,0> g=20000 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,2,0,2,0> g=20000 lds=6720 out=-1 in=-1 | PIPE<0,1,0,0,0,2,0,1,1> g=40000 lds=576 out=1 in=0"),
    (C(160000, E=12499968, bf16=True),
     "fam=PIPE f32=0 vec=1 wps=1 npw=2/2 pdl=0 eb=1 nt=0 rng=0 ell=0 defer=0 fc=3 L=4 | PIPE<1,0,1,0,1,0,0,2,0> g=20000 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,1,0,0,2,0> g=20000 lds=6720 out=-1 in=-1 | PIPE<0,1,1,0,1,0,0,1,0> g=40000 lds=6720 out=0 in=-1 | PIPE<0,1,0,0,1,0,0,1,0> g=40000 lds=576 out=1 in=-1"),
    (C(160000, E=12499969, bf16=True),
     "fam=PIPE f32=0 vec=1 wps=1 npw=2/2 pdl=0 eb=1 nt=1 rng=0 ell=0 defer=0 fc=3 L=4 | PIPE<1,0,1,0,1,1,0,2,0> g=20000 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,1,1,0,2,0> g=20000 lds=6720 out=-1 in=-1 | PIPE<0,1,1,0,1,1,0,1,0> g=40000 lds=6720 out=0 in=-1 | PIPE<0,1,0,0,1,1,0,1,0> g=40000 lds=576 out=1 in=-1"),
    (C(160000, E=21333312, bf16=True),
     "fam=PIPE f32=0 vec=1 wps=1 npw=1/1 pdl=0 eb=1 nt=1 rng=0 ell=0 defer=0 fc=3 L=4 | PIPE<1,0,1,0,1,1,0,1,0> g=40000 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,1,1,0,1,0> g=40000 lds=6720 out=-1 in=-1 | PIPE<0,1,1,0,1,1,0,1,0> g=40000 lds=6720 out=0 in=-1 | PIPE<0,1,0,0,1,1,0,1,0> g=40000 lds=576 out=1 in=-1"),
    (C(160000, E=21333313, bf16=True),
     "fam=PIPE f32=0 vec=1 wps=1 npw=1/1 pdl=0 eb=1 nt=2 rng=0 ell=0 defer=0 fc=3 L=4 | PIPE<1,0,1,0,1,2,0,1,0> g=40000 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,1,2,0,1,0> g=40000 lds=6720 out=-1 in=-1 | PIPE<0,1,1,0,1,2,0,1,0> g=40000 lds=6720 out=0 in=-1 | PIPE<0,1,0,0,1,2,0,1,0> g=40000 lds=576 out=1 in=-1"),
    (C(1024, tune=("pd_lds_min", 1)),
     "fam=PIPE f32=0 vec=1 wps=1 npw=1/1 pdl=1 eb=0 nt=0 rng=0 ell=0 defer=0 fc=3 L=4 | PIPE<1,0,1,1,0,0,0,1,0> g=256 lds=39520 out=-1 in=-1 | PIPE<0,0,1,1,0,0,0,1,0> g=256 lds=39520 out=-1 in=-1 | PIPE<0,1,1,1,0,0,0,1,0> g=256 lds=39520 out=0 in=-1 | PIPE<0,1,0,1,0,0,0,1,0> g=256 lds=33376 out=1 in=-1"),
    (C(1025, tune=("pd_lds_min", 1)),
     "fam=PIPE f32=0 vec=1 wps=1 npw=1/1 pdl=0 eb=0 nt=0 rng=0 ell=0 defer=0 fc=3 L=4 | PIPE<1,0,1,0,0,0,0,1,0> g=257 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,1,0> g=257 lds=6720 out=-1 in=-1 | PIPE<0,1,1,0,0,0,0,1,0> g=257 lds=6720 out=0 in=-1 | PIPE<0,1,0,0,0,0,0,1,0> g=257 lds=576 out=1 in=-1"),
    (C(1024, E=6249985, tune=("pd_lds_min", 1)),   # a non-temporal policy (150 MB of state) and the table: NT 0
     "fam=PIPE f32=0 vec=1 wps=4 npw=1/1 pdl=1 eb=0 nt=1 rng=0 ell=6112 defer=0 fc=3 L=4 | PIPE<1,0,1,1,0,0,0,1,0> g=1024 lds=39520 out=-1 in=-1 | PIPE<0,0,1,1,0,0,0,1,0> g=1024 lds=39520 out=-1 in=-1 | PIPE<0,1,1,1,0,0,0,1,0> g=1024 lds=39520 out=0 in=-1 | PIPE<0,1,0,1,0,0,0,1,0> g=1024 lds=33376 out=1 in=-1"),
    (C(1024, tune=("pd_lds_min", 1), bf16=True),
     "fam=PIPE f32=0 vec=1 wps=1 npw=1/1 pdl=1 eb=1 nt=0 rng=0 ell=0 defer=0 fc=3 L=4 | PIPE<1,0,1,1,1,0,0,1,0> g=256 lds=39520 out=-1 in=-1 | PIPE<0,0,1,1,1,0,0,1,0> g=256 lds=39520 out=-1 in=-1 | PIPE<0,1,1,1,1,0,0,1,0> g=256 lds=39520 out=0 in=-1 | PIPE<0,1,0,1,1,0,0,1,0> g=256 lds=33376 out=1 in=-1"),
    (C(512, tune=("pd_lds_min", 1)),
     "fam=FAST f32=1 vec=1 wps=1 npw=1/1 pdl=1 eb=0 nt=0 rng=0 ell=0 defer=0 fc=3 L=4 | FAST<1,0,1,1,0,0> g=128 lds=23104 out=-1 in=-1 | FAST<0,0,1,1,0,0> g=128 lds=23104 out=-1 in=-1 | FAST<0,1,1,1,0,0> g=128 lds=23104 out=0 in=-1 | FAST<0,1,0,1,0,0> g=128 lds=16960 out=1 in=-1"),
    # layout
    (C(16384, E=2 ** 19 - 1),
     "fam=PIPE f32=0 vec=1 wps=1 npw=2/2 pdl=0 eb=0 nt=0 rng=0 ell=0 defer=1 fc=3 L=4 | PIPE<1,0,1,0,0,0,0,2,0> g=2048 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,2,0> g=2048 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,2,0> g=2048 lds=6720 out=-1 in=-1 | PIPE<0,1,0,0,0,0,0,1,1> g=4096 lds=576 out=1 in=0"),
    (C(16384, E=2 ** 19),
     "fam=PIPE f32=0 vec=1 wps=1 npw=2/2 pdl=0 eb=0 nt=0 rng=0 ell=32 defer=1 fc=3 L=4 | PIPE<1,0,1,0,0,0,0,2,0> g=2048 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,2,0> g=2048 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,2,0> g=2048 lds=6720 out=-1 in=-1 | PIPE<0,1,0,0,0,0,0,1,1> g=4096 lds=576 out=1 in=0"),
    (C(18204, E=2 ** 19),
     "fam=PIPE f32=0 vec=1 wps=1 npw=2/2 pdl=0 eb=0 nt=0 rng=0 ell=32 defer=1 fc=3 L=4 | PIPE<1,0,1,0,0,0,0,2,0> g=2276 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,2,0> g=2276 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,2,0> g=2276 lds=6720 out=-1 in=-1 | PIPE<0,1,0,0,0,0,0,1,1> g=4551 lds=576 out=1 in=0"),
    (C(18409, E=2 ** 19),
     "fam=PIPE f32=0 vec=1 wps=1 npw=2/2 pdl=0 eb=0 nt=0 rng=0 ell=0 defer=1 fc=3 L=4 | PIPE<1,0,1,0,0,0,0,2,0> g=2302 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,2,0> g=2302 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,2,0> g=2302 lds=6720 out=-1 in=-1 | PIPE<0,1,0,0,0,0,0,1,1> g=4603 lds=576 out=1 in=0"),
    (C(16384, E=2 ** 19, unaligned=True),
     "fam=GEN f32=0 vec=0 wps=1 npw=2/2 pdl=0 eb=0 nt=0 rng=0 ell=0 defer=0 fc=3 L=4 | GEN<0,1,0> g=4096 lds=6656 out=-1 in=-1 | GEN<0,1,0> g=4096 lds=6656 out=-1 in=-1 | GEN<0,1,0> g=4096 lds=6656 out=0 in=-1 | GEN<0,0,0> g=4096 lds=512 out=1 in=-1"),
    # edges
    (C(513, L=0, cls=0),
     "fam=GEN f32=0 vec=1 wps=1 npw=1/1 pdl=0 eb=0 nt=0 rng=0 ell=0 defer=0 fc=1 L=0 | GEN<0,0,0> g=129 lds=512 out=0 in=-1"),
    (C(513, L=0, cls=0, reattach_edges=True),
     "fam=GEN f32=0 vec=1 wps=1 npw=1/1 pdl=0 eb=0 nt=0 rng=0 ell=0 defer=0 fc=1 L=0 | GEN<1,0,0> g=129 lds=512 out=0 in=-1"),
    (C(513, L=1, cls=1),
     "fam=PIPE f32=0 vec=1 wps=1 npw=1/1 pdl=0 eb=0 nt=0 rng=0 ell=0 defer=0 fc=1 L=1 | PIPE<1,1,0,0,0,0,0,1,0> g=129 lds=576 out=0 in=-1"),
    (C(512, L=1, cls=1),
     "fam=FAST f32=1 vec=1 wps=1 npw=1/1 pdl=0 eb=0 nt=0 rng=0 ell=0 defer=0 fc=1 L=1 | FAST<1,1,0,0,0,0> g=128 lds=576 out=0 in=-1"),
    (C(513, cls=4),
     "fam=PIPE f32=0 vec=1 wps=1 npw=1/1 pdl=0 eb=0 nt=0 rng=0 ell=0 defer=0 fc=1 L=4 | PIPE<1,1,1,0,0,0,0,1,0> g=129 lds=6720 out=0 in=-1 | PIPE<0,1,1,0,0,0,0,1,0> g=129 lds=6720 out=1 in=-1 | PIPE<0,1,1,0,0,0,0,1,0> g=129 lds=6720 out=2 in=-1 | PIPE<0,1,0,0,0,0,0,1,0> g=129 lds=576 out=3 in=-1"),
    (C(16384, cls=4),
     "fam=PIPE f32=0 vec=1 wps=1 npw=2/2 pdl=0 eb=0 nt=0 rng=0 ell=0 defer=1 fc=1 L=4 | PIPE<1,0,1,0,0,0,0,2,0> g=2048 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,2,1> g=2048 lds=6720 out=-1 in=0 | PIPE<0,0,1,0,0,0,0,2,1> g=2048 lds=6720 out=-1 in=1 | PIPE<0,1,0,0,0,0,0,1,1> g=4096 lds=576 out=3 in=2"),
    (C(513, L=9, cls=2),
     "fam=PIPE f32=0 vec=1 wps=1 npw=1/1 pdl=0 eb=0 nt=0 rng=0 ell=0 defer=0 fc=8 L=9 | PIPE<1,0,1,0,0,0,0,1,0> g=129 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,1,0> g=129 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,1,0> g=129 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,1,0> g=129 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,1,0> g=129 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,1,0> g=129 lds=6720 out=-1 in=-1 | PIPE<0,0,1,0,0,0,0,1,0> g=129 lds=6720 out=-1 in=-1 | PIPE<0,1,1,0,0,0,0,1,0> g=129 lds=6720 out=0 in=-1 | PIPE<0,1,0,0,0,0,0,1,0> g=129 lds=576 out=1 in=-1"),
    (C(513, E=0),
     "no steps"),
]

_PROBE = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "internal.h"
using namespace gnncca;
static void layer(gnncca_mlp& m, int in, int out) {
    gnncca_layer& l = m.layers[m.n_layers++];
    l.in_dim = in, l.out_dim = out, l.has_bn = 0, l.relu = out != 1;
}
int main(int argc, char** argv) {
    static const char* fams[] = {"GEN", "FAST", "PIPE"};
    for (int a = 1; a < argc; ++a) {
        int N = 0, E = 0, L = 0, C = 0, bits = 0;
        char field[64] = "";
        long long value = 0;
        const int got = std::sscanf(argv[a], "%d:%d:%d:%d:%d:%63[^=]=%lld", &N, &E, &L, &C, &bits, field, &value);
        if (got != 5 && got != 7) return 2;
        gnncca_mpn_dims d;
        std::memset(&d, 0, sizeof(d));
        d.abi_version = GNNCCA_ABI_VERSION, d.node_in = 2048, d.edge_in = (bits & 8) ? 5 : 4, d.node_dim = kH, d.edge_dim = kEF;
        d.agg = (bits & 4) ? GNNCCA_AGG_MAX : GNNCCA_AGG_SUM;
        d.num_enc_steps = L, d.num_class_steps = C, d.reattach_edges = (bits & 16) != 0, d.reattach_nodes = (bits & 32) != 0;
        layer(d.enc_node, 2048, 128), layer(d.enc_node, 128, kH);
        const int nf = d.reattach_nodes ? 2 : 1, ef = d.reattach_edges ? 2 : 1;
        layer(d.enc_edge, d.edge_in, kEF), layer(d.edge_mlp, nf * 2 * kH + ef * kEF, kEF), layer(d.node_mlp, nf * kH + kEF, kH);
        layer(d.cls_edge, kEF, 4), layer(d.cls_edge, 4, 1);
        BlobHeader hdr;
        if (!blob_header(&d, &hdr)) return 3;
        const Workspace ws = carve(&d, N, E);
        StepTuning t;
        struct { const char* name; int* at; } fields[] = {{"force_wps", &t.force_wps}, {"force_npw", &t.force_npw}, {"force_nt", &t.force_nt},
            {"npw_min_n", &t.npw_min_n}, {"npw_min_n_first", &t.npw_min_n_first}, {"pd_lds_min", &t.pd_lds_min}, {"pd_lds_max", &t.pd_lds_max}};
        bool known = !field[0];
        for (auto& f : fields)
            if (!std::strcmp(f.name, field)) *f.at = (int)value, known = true;
        if (!known) return 4;
        const uint32_t options = (bits & 256 ? GNNCCA_OPT_ENC_UNSPLIT : 0) | (bits & 512 ? GNNCCA_OPT_EDGE_STATE_BF16 : 0) |
                                 (bits & 1024 ? GNNCCA_OPT_COLUMN_RANGES : 0);
        const StepRouteIn in{&d, &hdr, &ws, N, E, options, (bits & 128) != 0, (bits & 1) != 0, (bits & 2) != 0, !(bits & 64)};
        const StepPlan p = step_plan(in, t);
        if (p.launches == 0) {
            std::printf("no steps\n");
            continue;
        }
        std::printf("fam=%s f32=%d vec=%d wps=%d npw=%d/%d pdl=%d eb=%d nt=%d rng=%d ell=%d defer=%d fc=%d L=%d", fams[p.family], p.msg_f32, p.attr_vec,
                    p.wps, p.npw_first, p.npw_later, p.pd_lds, p.e_bf16, p.nt, (int)p.ranges, p.ell_S, (int)p.defer, p.first_cls, p.L);
        char tail[1024] = "";
        for (int i = 0; i < p.launches; ++i) {
            const int step = p.L == 0 ? 0 : i + 1;
            const StepLaunch l = step_launch(p, step);
            if (l.family == kStepGeneral) std::printf(" | GEN<%d,%d,%d>", l.RE, l.MSG, l.MX);
            else if (l.family == kStepFast) std::printf(" | FAST<%d,%d,%d,%d,%d,%d>", l.FIRST, l.CLS, l.MSG, l.PDL, l.EB, l.NT);
            else std::printf(" | PIPE<%d,%d,%d,%d,%d,%d,%d,%d,%d>", l.FIRST, l.CLS, l.MSG, l.PDL, l.EB, l.NT, l.RNG, l.NPW, l.CIN);
            std::printf(" g=%u lds=%zu out=%d in=%d", l.blocks, l.lds, l.slot_out, l.slot_in);
            // behind the '#': store_e : table read > written : first . update . npw . cls_layers . cls_no . stamp_slot : exists
            std::snprintf(tail + std::strlen(tail), sizeof(tail) - std::strlen(tail), " %d:%d>%d:%d.%d.%d.%d.%d.%d:%d", l.store_e, l.buf_in, l.buf_out,
                          l.first, l.update, l.npw, l.cls_layers, l.cls_no, l.stamp_slot,
                          (int)step_variant_exists(l.family, l.FIRST, l.CLS, l.MSG, l.PDL, l.EB, l.NT, l.RNG, l.NPW, l.CIN));
        }
        std::printf(" #%s\n", tail);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("step_route")
    src, exe = tmp / "probe.cpp", tmp / "probe"
    src.write_text(_PROBE)
    subprocess.run([_host_compiler(), "-std=c++17", "-O0", "-I", os.path.join(ROOT, "include"), "-I", CSRC, str(src),
                    os.path.join(CSRC, "step_route.cpp"), os.path.join(CSRC, "pack.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)] + [c for c, _ in TABLE], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(TABLE)
    return dict(zip((c for c, _ in TABLE), out))


@pytest.mark.parametrize("case,want", TABLE)
def test_route_is_the_table(routes, case, want):
    got = routes[case]
    assert got.split(" #", 1)[0] == want, (case, got)


def test_no_edges_do_not_reach_the_steps(routes):
    assert routes[C(513, E=0)] == "no steps"


@pytest.mark.parametrize("case", [c for c, w in TABLE if w != "no steps"])
def test_steps_fit_together(routes, case):
    """Every named instantiation is one the library has (step_variant_exists); every logit slot 0 .. n_class - 1 is written exactly once
    over the forward, counting the slots classified from a step's input state; every step but the last stores the edge state; the
    per-node projection tables alternate: a step reads the table the step before it wrote."""
    got = routes[case]
    head, tail = got.split(" #", 1)
    L, fc = (int(re.search(rf" {k}=(-?\d+)", head).group(1)) for k in ("L", "fc"))
    steps = [re.match(r"(\d):(-?\d+)>(-?\d+):[\d.]+:(\d)$", s).groups() for s in tail.split()]
    assert len(steps) == max(L, 1) and all(s[3] == "1" for s in steps), got
    slots = sorted(int(v) for v in re.findall(r" (?:out|in)=(\d+)", head))
    n_class = 1 if L == 0 else L - max(fc, 1) + 1
    assert slots == list(range(n_class)), got
    assert [s[0] for s in steps] == ["1"] * (len(steps) - 1) + ["0"], got
    if L > 0:
        assert [(s[1], s[2]) for s in steps] == [(str((i - 1) & 1), str(i & 1) if i < L else "-1") for i in range(1, L + 1)], got
