"""GPU: the MSM's bucket stages on the designed bucket occupancies of tests/msm_occupancy.py -- staircases of adjacent mid-size buckets,
sizes around every power of two, bucket ends on and off the lane ends of the accumulate walk at every phase, both ends of a bucket set
heavy, every bucket of a small set in play, the bit-and-nibble witness in small, and equal / opposite points inside a bucket including
the levels' own stand-in point -- under every number of regular (MNT753_MSM_PAIR) and irregular (MNT753_MSM_IRR) batched-affine levels,
every floor of entries per lane (MNT753_MSM_TMIN), the three sort stages and both forms of the edge-tree levels.  Every comparison is
a bit-exact group element.

The cases and their knob settings are msm_occupancy.all_cases(): the list tests/test_msm_occupancy_cpu.py proves to reach every event of
the host model.  One base set per case; the knobs are read on every MSM, so a case loops over them, checks after every MSM that the
plan the library reports is the one asked for (a setting it silently replaced would pass for the wrong reason) and fails with the
list of all settings whose plan or result differs.

Two pieces of the library's state outlive an MSM on a base set.  The level buffers grow with the largest PAIR seen, and an
irregular level that does not fit them is dropped: the reported irr_levels is the number that RAN, so the plan check sees it.  The
partition sort's buffers exist only if the workspace was last rebuilt under a setting that asks for that sort; an MSM that asks for
it without them takes the atomic sort, and the sort stage is NOT reported, so it is not checked on the device.  The settings of a case
therefore run in the order msm_occupancy.run_order gives them -- partition sorts before atomic, largest PAIR first -- and
tests/test_msm_occupancy_cpu.py proves from a restatement of those host rules that in this order every part / generic setting sorts
by partition and every setting has room for all the irregular levels it asks for.  (At c = 12 `part` and `generic` are the same
passes, the ones that read the width at run time; the passes by width start at c = 14 and belong to tests/test_msm_structured_gpu.py.)

The expectation comes through the discrete logs of the synthetic bases
(synth_expected_msm); `collisions`, whose bases are replaced by copies, negatives and +-G, takes it from the oracle's multi-exp -- the
CPU file pins both to each other.

Seconds per case on an MI355X, measured once (pytest --durations, call phase: profile, expectation, base set with its window table and
all MSMs of the case; an MSM of these sizes is about 3 ms), nothing thinned:
    test_g1_table_mode, the six profiles (60 MSMs each)                      0.18 .. 0.24
    test_g1_table_mode, aligned_T* (13 MSMs) and aligned_blocked_L* (12 .. 16) 0.05 .. 0.09
    test_g2_table_mode (3 .. 6 MSMs; MNT6753 the slower)                     0.06 .. 0.11
    test_g1_full_set (9 MSMs)                                                0.04 .. 0.05
    test_g1_without_the_table (6 MSMs)                                       0.02 .. 0.03
    the whole file: 76 cases, 1354 MSMs, in 7.4 s
"""
import numpy as np
import pytest

import msm_occupancy as M
import msm_structured as S
import oracle_lib as O

pytestmark = pytest.mark.gpu

_SYNTH = {}
SYNTH_MAX = {1: 1024, 2: 512}


def seed_of(curve, group):
    return 9700 + 10 * curve + group


def synth(gpu, curve, group, n):
    """the synthetic bases of (curve, group): generated once per module run, shared read-only (base k is the same point at every n)"""
    key = (curve, group)
    if key not in _SYNTH:
        a = gpu.synth_points(curve, group, seed_of(curve, group), SYNTH_MAX[group])
        a.setflags(write=False)
        _SYNTH[key] = a
    assert n <= SYNTH_MAX[group]
    return _SYNTH[key][:n]


def negate(curve, group, p):
    h = p.size // 2
    out = p.copy()
    out[h:] = O.neg_fq(curve, p[h:]) if group == 1 else O.ext_op(curve, 5, p[h:])
    return out


def bases_and_expectation(gpu, curve, group, prof):
    """(affine base points, scalars in wire form, expected affine words)"""
    sc = S.wire(curve, prof.ints)
    pts = synth(gpu, curve, group, len(prof.ints))
    if prof.recipe is None:
        want = gpu.point_to_affine(curve, group, gpu.synth_expected_msm(curve, group, seed_of(curve, group), sc))
    else:
        pts = M.apply_recipe(prof.recipe, pts, gpu.api.test_generator(curve, group), lambda p: negate(curve, group, p))
        want = O.msm(curve, group, pts, sc)
    assert want.any()                          # no profile sums to the identity: a result of zeros is never right
    return pts, sc, want


ENV = dict(pair="MNT753_MSM_PAIR", irr="MNT753_MSM_IRR", tmin="MNT753_MSM_TMIN", sort="MNT753_MSM_SORT", edge_flow="MNT753_EDGE_FLOW_NODES")


def set_knobs(monkeypatch, knob):
    for k, name in ENV.items():
        if k in knob:
            monkeypatch.setenv(name, str(knob[k]))
        else:
            monkeypatch.delenv(name, raising=False)


def run_case(gpu, monkeypatch, curve, group, cs):
    prof = cs.build(curve)
    pts, sc, want = bases_and_expectation(gpu, curve, group, prof)
    n, lanes = len(prof.ints), M.lanes_per_point(curve, group)
    set_knobs(monkeypatch, cs.knobs[0])         # the base set sizes its workspace and level buffers for the first setting (M.run_order)
    bs = gpu.BaseSet(curve, group, pts)
    bad = []
    try:
        for knob in cs.knobs:
            set_knobs(monkeypatch, knob)
            got = gpu.point_to_affine(curve, group, bs.msm(sc))
            plan = gpu.msm_last_plan()
            asked = dict(window_table=cs.table, window_bits=cs.c, windows=S.windows(cs.c), entries_per_lane=M.plan_T(n, cs.c, lanes, knob["tmin"]),
                         pair_levels=knob["pair"], irr_levels=knob["irr"])
            if plan != asked:
                bad.append((knob, "the library ran another plan", plan))
            elif not np.array_equal(got, want):
                bad.append((knob, "wrong group element"))
    finally:
        bs.close()
    assert not bad, f"curve {curve}, G{group}, {cs.name} (n = {n}, c = {cs.c}, table {cs.table}): {len(bad)} of {len(cs.knobs)} settings fail: {bad}"


def ids(cases):
    return [cs.name for cs in cases]


# ---- G1, one bucket set shared by all windows, c = 12 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("cs", M.g1_cases(), ids=ids(M.g1_cases()))
@pytest.mark.parametrize("curve", [0, 1])
def test_g1_table_mode(gpu, monkeypatch, curve, cs):
    """PAIR in {0, 1, 2, 3, 6} x IRR in {0, 1, 3} x TMIN in {1, 3, 4, 8} under the partitioned sort (52 MSMs), the other sort stages and both
    forms of the edge-tree levels at two fixed settings; aligned(T, phase) at TMIN = T, aligned(8 * 2^L, phase) behind L levels"""
    monkeypatch.setenv("MNT753_MSM_PRECOMP", "1")
    monkeypatch.setenv("MNT753_MSM_TABLE_BITS", str(cs.c))
    run_case(gpu, monkeypatch, curve, 1, cs)


@pytest.mark.parametrize("curve", [0, 1])
def test_g1_full_set(gpu, monkeypatch, curve):
    """c = 8: W = 95 windows over 128 buckets, every one of them in play; the atomic sort (the partition passes do not apply)"""
    cs = M.full_set_case()
    monkeypatch.setenv("MNT753_MSM_PRECOMP", "1")
    monkeypatch.setenv("MNT753_MSM_TABLE_BITS", str(cs.c))
    run_case(gpu, monkeypatch, curve, 1, cs)


@pytest.mark.parametrize("cs", M.no_table_cases(), ids=ids(M.no_table_cases()))
@pytest.mark.parametrize("curve", [0, 1])
def test_g1_without_the_table(gpu, monkeypatch, curve, cs):
    """c = 7, one bucket set per window (key = w nb + |d| - 1): the staircase in set 0, in set 100 with 6336 empty keys in front of it,
    and both ends of set 0 heavy with the carries in set 1"""
    monkeypatch.setenv("MNT753_MSM_PRECOMP", "0")
    monkeypatch.delenv("MNT753_MSM_TABLE_BITS", raising=False)
    old = gpu.lib().mnt753_msm_set_window_bits(cs.c)
    try:
        run_case(gpu, monkeypatch, curve, 1, cs)
    finally:
        gpu.lib().mnt753_msm_set_window_bits(old)


# ---- G2: the lane-split kernels ----------------------------------------------------------------------------------------------------------
G2_CASES = [(curve, cs) for curve in (0, 1) for cs in M.g2_cases(curve)]


@pytest.mark.parametrize("curve,cs", G2_CASES, ids=[f"{curve}-{cs.name}" for curve, cs in G2_CASES])
def test_g2_table_mode(gpu, monkeypatch, curve, cs):
    """two (Fq2) / three (Fq3) lanes per point: every profile at its G2 size, PAIR in {0, 2} x IRR in {0, 2} x TMIN in {1, 8}"""
    monkeypatch.setenv("MNT753_MSM_PRECOMP", "1")
    monkeypatch.setenv("MNT753_MSM_TABLE_BITS", str(cs.c))
    run_case(gpu, monkeypatch, curve, 2, cs)
