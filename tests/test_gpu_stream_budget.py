"""The coefficient op's pipeline on TWO internal streams: how many streams the library keeps (sr_stream_census) and that
the pipelined schedule computes what the serial one does, bit for bit, with four hardware queues as with eight.

Every GPU step is a fresh child process with its own timeout (GPU_MAX_HW_QUEUES is read once, at the process's first
HIP call, and the census counts per process).

Line densities matter here.  In the default far-field mode a line set with fewer than 0.35 lines per grid point takes the
per-line expansions (far_st: prep -> level-0 pass, the zones kernel released by the end of that chain), a denser one the
box pairs (far_st: prep -> level-0 pass -> S2M, M2M -> M2L, moments and coefficients per parity, the zones kernel released
behind S2M) -- the headline's path.  DENSE lists (12000 lines on 20000 points: 0.6; their ground-state sub-lineset 0.48,
so a level-table build sends it through a private CoefWork) are what these tests are about; the sparse pipeline runs
beside them.  Each child reports the densities it ran at and the tests assert on which side of 0.35 they lie."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPARSE_BELOW = 0.35   # lines per grid point (coef_op's and mc_pass's rule in far-field mode 3)

_PRELUDE = r"""
import ctypes as C, json, sys
sys.path.insert(0, %r)
import numpy as np
import torch
from spectrobot_amd import engine, synthetic as syn
from spectrobot_amd._lib import lib

def census():
    live, total = C.c_int(-1), C.c_int(-1)
    assert lib.sr_stream_census(C.byref(live), C.byref(total)) == 0
    return [live.value, total.value]

NG = 20000
engine.set_device(0)
grid = syn.make_grid(2988.0, 5e-4, NG)

def lineset(n_lines, seed):
    L = syn.make_lines(n_lines, grid, seed=seed, n_levels=12)
    ls = engine.LineSet(L, grid, 6, 1, syn.CH4_MM, syn.CH4_LEVEL_ENERGIES)
    # (the lines the library kept; the per-level counts are of the input, which the filter can only lower)
    ground = int(np.count_nonzero((L["lev_up"] == 0) | (L["lev_lo"] == 0))) - (n_lines - ls.n_kept)
    others = max(int(np.count_nonzero((L["lev_up"] == lv) | (L["lev_lo"] == lv))) for lv in range(1, 12))
    return ls, dict(all=ls.n_kept / NG, ground=ground / NG, densest_other_level=others / NG)
""" % ROOT

_CENSUS = _PRELUDE + r"""
res = {"start": census()}
ls, res["density"] = lineset(12000, 17)
atm = syn.make_atmosphere(10, 12)
keep = []
for c in range(6):
    keep.append(ls.abscoeff_layers(atm["temps"] + 0.5 * c, atm["press"], tvib=atm["tvib"] + 0.5 * c))
res["after_coef"] = census()
Lr = syn.limb_los(atm["z"], syn.number_density(atm["press"], atm["temps"]), [np.full(10, 0.0148)], [atm["z"][0] + 5.0])
los = engine.LimbLOS(Lr["seg_off"], Lr["seg_layer"], Lr["pt_off"], Lr["x"], Lr["nd"], Lr["vmr"], col_scale=[syn.CH4_ISO_RATIO])
rad = engine.limb_rays(keep[-1], los)
res["after_los"] = census()
# default mode: the dense ground-state pass through a private CoefWork, the eleven sparse ones in the batch
keep.append(ls.glevel_pairs(atm["temps"], atm["press"]))
res["after_tables"] = census()
# box pairs for EVERY sub-lineset: all twelve far-only passes through the private CoefWorks, no sparse batch
try:
    engine.set_far_field(2)
    keep.append(ls.glevel_pairs(atm["temps"], atm["press"]))
finally:
    engine.set_far_field(engine.FAR_FIELD_DEFAULT)
res["after_tables_all_private"] = census()
torch.cuda.synchronize()
t = keep[-2]
res["tables_finite"] = bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0.0
los.close()
ls.close()
res["after_close"] = census()
print("RESULT " + json.dumps(res))
"""

# 8 consecutive calls with a changing atmosphere (a stale table set, or moments / coefficients of the wrong parity, show),
# alternating between two caller streams, pipelined and serial; plain, with frozen region boundaries, on a 1/8 shard
_BITWISE = _PRELUDE + r"""
ls, density = lineset(N_LINES, 7)
atm = syn.make_atmosphere(10, 12)
streams = [torch.cuda.Stream(), torch.cuda.Stream()]

def run(overlap, lo, hi):
    engine.set_overlap(overlap)
    out = []
    for c in range(8):
        with torch.cuda.stream(streams[c % 2]):
            out.extend(ls.abscoeff_layers(atm["temps"] + 0.7 * c, atm["press"] * (1.0 + 0.01 * c), tvib=atm["tvib"] + 0.4 * c,
                                          g_lo=lo, g_hi=hi))
    torch.cuda.synchronize()
    return out

res = {"density": density}
try:
    for name, lo, hi, frozen in (("plain", 0, NG, False), ("frozen", 0, NG, True), ("shard", 3 * NG // 8, 4 * NG // 8, False)):
        ls.set_bounds_temps(atm["temps"] if frozen else None)
        a = run(1, lo, hi)
        b = run(0, lo, hi)
        res[name] = [bool(torch.equal(x, y)) for x, y in zip(a, b)]
        res[name + "_finite"] = bool(all(torch.isfinite(x).all() and float(x.abs().max()) > 0.0 for x in a[:2]))
        res[name + "_changing"] = not bool(torch.equal(a[0], a[2]))
finally:
    engine.set_overlap(1)
    ls.set_bounds_temps(None)
res["census"] = census()
print("RESULT " + json.dumps(res))
"""

_TWO_HANDLES = _PRELUDE + r"""
sets, density = [], []
for seed, n in ((7, 12000), (11, 9000), (13, 5000)):     # two on the box-pair pipeline, one on the per-line one
    ls, d = lineset(n, seed)
    sets.append(ls)
    density.append(d["all"])
atm = syn.make_atmosphere(10, 12)
streams = [torch.cuda.Stream(), torch.cuda.Stream()]

def run(overlap):
    engine.set_overlap(overlap)
    out = [[] for _ in sets]
    for c in range(6):
        for k in range(len(sets)):
            with torch.cuda.stream(streams[(c + k) % 2]):
                out[k].extend(sets[k].abscoeff_layers(atm["temps"] + 0.7 * c, atm["press"], tvib=atm["tvib"] + 0.4 * c))
    torch.cuda.synchronize()
    return out

try:
    a = run(1)
    b = run(0)
finally:
    engine.set_overlap(1)
res = {"set%d" % k: [bool(torch.equal(x, y)) for x, y in zip(a[k], b[k])] for k in range(len(sets))}
res["density"] = density
res["differ"] = not bool(torch.equal(a[0][0], a[1][0]))
res["census"] = census()
print("RESULT " + json.dumps(res))
"""


def _child(code, queues=None, timeout=240):
    env = dict(os.environ)
    if queues is not None:
        env["GPU_MAX_HW_QUEUES"] = str(queues)
    p = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       universal_newlines=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-4000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
    assert len(lines) == 1, p.stdout[-4000:]
    return json.loads(lines[0][7:])


@pytest.mark.gpu
def test_library_keeps_at_most_three_streams():
    """Six pipelined coefficient calls on a DENSE list (box-pair pipeline), a LimbLOS (+ one limb_rays, which stages
    early) and two level-table builds on one lineset: at most 3 library-made streams live (2 pipeline + 1 staging) and no
    more than 3 ever created.  The first build sends the dense ground-state sub-lineset through a private CoefWork
    (McWork::fw) and the sparse ones through the batch; the second (box pairs forced for every sub-lineset) sends all
    twelve through the private CoefWorks -- each of which would make a pair of its own on its first pipelined call if it
    did not borrow the handle's (no extra stream was kept for them).  Destroying the handles destroys the two pipeline
    streams; the thread's staging stream stays."""
    r = _child(_CENSUS)
    print(r)
    d = r["density"]
    assert d["all"] > SPARSE_BELOW and d["ground"] > SPARSE_BELOW > d["densest_other_level"], d
    assert r["start"] == [0, 0]
    for k in ("after_coef", "after_los", "after_tables", "after_tables_all_private"):
        assert 2 <= r[k][0] <= 3 and r[k][1] <= 3, (k, r)
    assert r["tables_finite"]
    assert r["after_close"][0] == r["after_tables_all_private"][0] - 2 and r["after_close"][0] <= 1, r
    assert r["after_close"][1] <= 3, r


@pytest.mark.gpu
@pytest.mark.parametrize("n_lines", [12000, 6000], ids=["box-pairs", "per-line"])
@pytest.mark.parametrize("queues", [4, 8])
def test_pipelined_equals_serial_bitwise(queues, n_lines):
    r = _child(_BITWISE.replace("N_LINES", str(n_lines)), queues=queues)
    print(r)
    assert (r["density"]["all"] > SPARSE_BELOW) == (n_lines == 12000) and r["density"]["all"] > 0.25, r["density"]
    for name in ("plain", "frozen", "shard"):
        assert len(r[name]) == 16 and all(r[name]), (name, r)
        assert r[name + "_finite"] and r[name + "_changing"], (name, r)
    assert r["census"][0] <= 3, r


@pytest.mark.gpu
def test_linesets_interleaved_on_two_streams():
    """Three top-level linesets (two pipeline streams each; two of them dense), their calls interleaved on two caller
    streams: each equals its own serial result bit for bit."""
    r = _child(_TWO_HANDLES)
    print(r)
    assert r["density"][0] > SPARSE_BELOW and r["density"][1] > SPARSE_BELOW > r["density"][2], r["density"]
    for k in ("set0", "set1", "set2"):
        assert len(r[k]) == 12 and all(r[k]), (k, r)
    assert r["differ"]
    assert r["census"][0] <= 7, r                  # 3 x 2 pipeline streams, at most one staging stream
