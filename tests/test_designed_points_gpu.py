"""GPU: the group-law kernels on the points with designed coordinates of tests/designed_points.py -- stored x values whose low limbs
collide (the quick zero test of k_pair_level fires and has to be settled as "not zero"), points on one horizontal line (lambda = 0 in the
affine pair addition, u = 0 with v != 0 in the projective ones), G2 points whose x agrees with the other operand's in some components
only (the lanes of one point disagree about "zero" until they are combined), neighbours, sparse coordinates and coordinates at the edges
of the representation.  Every comparison is a bit-exact group element; every expectation is the CPU oracle's
(tests/test_designed_points_cpu.py pins the oracle to tools/pyref.py on the same inputs).

a. Every form of the group law (mnt753_test_point_op: 0, 2, 3, 4, 5, 6 -- the forms and the combinations left out are those of
   tests/test_device_kat_gpu.py: the two-lanes addition has no one-lane G2 form, the lane-group addition is instantiated with the one-lane
   configuration), all pairs of a group in one launch per form: with Z = 1 and with each operand replaced by (lam X, lam Y, lam Z), lam in
   {q - 1, a uniform element, 1 / X}; for partial_x lam stays in the base field, so the partial zero survives.  A representative of Q goes
   to the full additions only (the mixed ones read Q as an affine point).  The doubling (op 1) on every designed point.
b. The affine pair addition of the levels and the accumulate walk, through MSMs in which every pair has a bucket of its own
   (designed_points.pair_bucket_input), a second copy with the second base flagged negative: PAIR in {0 .. 3} x IRR in {0, 1} x sort in
   {part, atomic} x TMIN in {1, 8}; G1 with the window table (c = 12) and without it (c = 7: the partition passes do not apply there, so the
   `part` half of the list repeats the `atomic` half), G2 with it and PAIR in {0, 2}.  The settings
   run in msm_occupancy.run_order and the plan the library reports is checked after every MSM, as in tests/test_msm_occupancy_gpu.py: a
   setting it replaced fails the case.
   What the first level reads: without the table, exactly what k_bases_to_internal stored.  With it, the row of window 0 -- and
   k_precompute_windows writes rows for w >= 1 only, "row 0 is the base itself (d_aff)": the same words.  The scalars here are below
   2^(c-1), digits of window 0, so the low-limb collision holds by construction in both modes (the carries of the flagged copy are the
   only rows of window 1, in bucket 1, apart from the pairs).  test_low_limb_fires_on_the_device confirms on the device, through the chain
   of the level (from_wire, sub_raw, raw_maybe_zero; sub, is_zero), that every low_limb pair fires the quick test and is not zero.
c. The full additions of the reduction: P alone in one bucket, Q alone in the bucket whose key differs in bit l, everything else empty,
   for every l < c - 1 at c = 8 and c = 12 -- whichever halving step joins the two adds exactly P + Q --, on the same_y, partial_x and
   edge_x pairs and on `opposite` -- (P, -P), a family beyond the three asked for: v = 0 with u != 0 is the other half of every
   `same = is_zero(u) && is_zero(v)`, and an on-curve pair with equal x and different y is a point and its negative --; and the edge
   merge: one bucket of 2T + 1 entries at T = 1 and 4 that holds P, Q and copies of a third point.
d. mnt753_check_points reports (0, 0, 0) on every family.

Seconds per test on an MI355X, measured once (pytest --durations, call phase), nothing thinned.  (Measured with 53 pairs on G2 of
MNT6753, before its sparse points were paired with each other: 62 now, so its rows below grow by a sixth.)
    test_group_law_on_designed_points (156 .. 532 rows per launch)            0.01 .. 0.02; the first form of a group builds its rows and
                                                                              their expectations: 0.14 .. 0.17 (G1), 0.30 / 0.57 (G2)
    test_doubling_of_designed_points                                          0.01 .. 0.02
    test_low_limb_fires_on_the_device, test_check_points_accepts_every_family below 0.005
    test_pair_buckets_table_mode (28 MSMs; G2: 12)                            0.10 .. 0.13
    test_pair_buckets_without_the_table (28 MSMs)                             0.08
    test_reduction_adds_two_lone_buckets, c = 8 (7 MSMs per pair)             0.25 .. 0.40
    test_reduction_adds_two_lone_buckets, c = 12 (11 MSMs per pair: 528 on G1) 0.48 (G1) .. 0.78 (G2 of MNT6753)
    test_edge_merge_of_designed_points (2 MSMs per pair)                      0.12 .. 0.24
    the whole file: 62 tests in 7.0 s, the designed points (built once per process, 3 s) included
"""
import functools

import numpy as np
import pytest

import designed_points as D
import msm_occupancy as M
import msm_structured as S
import oracle_lib as O

pytestmark = pytest.mark.gpu

GROUPS = [(0, 1), (1, 1), (0, 2), (1, 2)]
CONFIGS = [(0, 1, 0), (1, 1, 0), (0, 2, 0), (0, 2, 1), (1, 2, 0), (1, 2, 1)]        # (curve, group, lane-split form)
FORMS = {0: "VM addition", 2: "VM mixed addition", 3: "straight-line mixed addition", 4: "two point-lanes per addition", 5: "straight-line addition",
         6: "one group of lanes per addition"}
MIXED = (2, 3)


ENV = dict(pair="MNT753_MSM_PAIR", irr="MNT753_MSM_IRR", tmin="MNT753_MSM_TMIN", sort="MNT753_MSM_SORT", edge_flow="MNT753_EDGE_FLOW_NODES")


def set_knobs(monkeypatch, knob):
    """the knobs of tests/test_msm_occupancy_gpu.py: read on every MSM; a knob a setting does not name is unset"""
    for k, name in ENV.items():
        if k in knob:
            monkeypatch.setenv(name, str(knob[k]))
        else:
            monkeypatch.delenv(name, raising=False)


def form_exists(group, split, form):
    return not (form == 4 and group == 2 and not split) and not (form == 6 and split)


LAW = [(curve, group, split, form) for curve, group, split in CONFIGS for form in sorted(FORMS) if form_exists(group, split, form)]


# ---- a. every form of the group law -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def law_rows(curve, group):
    """[(label, P projective words, Q projective words, expected affine words, Q has Z = 1)], computed once per group"""
    rows = []
    k = 0
    for fam, mem in D.families_points(curve, group).items():
        for (name, P, Q), m in zip(mem, D.families(curve, group)[fam]):
            want = O.point_op(curve, group, 0, m.P, m.Q)
            want.setflags(write=False)
            p1, q1 = D.proj_words(curve, group, P), D.proj_words(curve, group, Q)
            rows.append((f"{name} Z=1", p1, q1, want, True))
            for side, pt in (("P", P), ("Q", Q)):
                k += 1
                for lname, lam in D.lambdas(curve, group, fam, pt, 5100 + k).items():
                    rep = D.proj_words(curve, group, pt, lam)
                    rows.append((f"{name} {side}*{lname}", rep if side == "P" else p1, rep if side == "Q" else q1, want, side == "P"))
    return rows


@pytest.mark.parametrize("curve,group,split,form", LAW)
def test_group_law_on_designed_points(gpu, curve, group, split, form):
    rows = [r for r in law_rows(curve, group) if r[4] or form not in MIXED]
    P = np.stack([r[1] for r in rows]); Q = np.stack([r[2] for r in rows])
    got = gpu.api.test_point_op(curve, group, split, form, P, Q).reshape(len(rows), -1)
    bad = [r[0] for r, g in zip(rows, got) if not np.array_equal(gpu.point_to_affine(curve, group, g), r[3])]
    assert not bad, f"{FORMS[form]}: {len(bad)} of {len(rows)} wrong: {bad[:12]}"


@pytest.mark.parametrize("curve,group,split", CONFIGS)
def test_doubling_of_designed_points(gpu, curve, group, split):
    pts = D.distinct_points(curve, group)
    want = [O.point_op(curve, group, 1, D.to_words(curve, group, pt)) for pt in pts]
    reps = [D.proj_words(curve, group, pt) for pt in pts]
    reps += [D.proj_words(curve, group, pt, D.lambdas(curve, group, "", pt, 6100 + k)["uniform"]) for k, pt in enumerate(pts)]
    got = gpu.api.test_point_op(curve, group, split, 1, np.stack(reps)).reshape(len(reps), -1)
    bad = [k for k, g in enumerate(got) if not np.array_equal(gpu.point_to_affine(curve, group, g), want[k % len(pts)])]
    assert not bad, f"doubling: rows {bad} of {len(reps)} wrong (the second half are the scaled representatives)"


# ---- b. every pair in a bucket of its own ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", [0, 1])
def test_low_limb_fires_on_the_device(gpu, curve):
    """the chain of the first level on the device, bit-identical to the model (fp_norm is not involved): maybe zero, not zero"""
    mem = D.families_points(curve, 1)["low_limb"]
    maybe, zero, l1, l2 = D.low_limb_chain(gpu.api.test_field_raw, curve, [(P[0], Q[0]) for _, P, Q in mem])
    for i, (name, P, Q) in enumerate(mem):
        assert [int(w) for w in l1[i]] == D.stored_limbs(curve, P[0]) and [int(w) for w in l2[i]] == D.stored_limbs(curve, Q[0]), name
    assert maybe.all() and not zero.any(), (maybe, zero)


def run_settings(gpu, monkeypatch, curve, group, cs, pts, sc, want):
    """the loop of test_msm_occupancy_gpu.run_case on given bases: one base set, every setting of the case, the plan checked"""
    n, lanes = len(pts), M.lanes_per_point(curve, group)
    set_knobs(monkeypatch, cs.knobs[0])
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


def table_mode(monkeypatch, c):
    monkeypatch.setenv("MNT753_MSM_PRECOMP", "1")
    monkeypatch.setenv("MNT753_MSM_TABLE_BITS", str(c))


@pytest.mark.parametrize("curve,group", GROUPS)
def test_pair_buckets_table_mode(gpu, monkeypatch, curve, group):
    cs = D.pair_bucket_cases(curve, group)[0]
    pts, ints, _ = cs.build(curve)
    sc = S.wire(curve, ints)
    table_mode(monkeypatch, cs.c)
    run_settings(gpu, monkeypatch, curve, group, cs, pts, sc, O.msm(curve, group, pts, sc))


@pytest.mark.parametrize("curve", [0, 1])
def test_pair_buckets_without_the_table(gpu, monkeypatch, curve):
    cs = D.pair_bucket_cases(curve, 1)[1]
    pts, ints, _ = cs.build(curve)
    sc = S.wire(curve, ints)
    monkeypatch.setenv("MNT753_MSM_PRECOMP", "0")
    monkeypatch.delenv("MNT753_MSM_TABLE_BITS", raising=False)
    old = gpu.lib().mnt753_msm_set_window_bits(cs.c)
    try:
        run_settings(gpu, monkeypatch, curve, 1, cs, pts, sc, O.msm(curve, 1, pts, sc))
    finally:
        gpu.lib().mnt753_msm_set_window_bits(old)


# ---- c. the full additions of the reduction, the edge merge -----------------------------------------------------------------------------------
def check_plan(gpu, c, T):
    plan = gpu.msm_last_plan()
    return plan["window_table"] and plan["window_bits"] == c and plan["entries_per_lane"] == T and plan["pair_levels"] == 0


@pytest.mark.parametrize("c", [8, 12])
@pytest.mark.parametrize("curve,group", GROUPS)
def test_reduction_adds_two_lone_buckets(gpu, monkeypatch, curve, group, c):
    """c = 8: the full-set geometry (128 buckets, the atomic sort: the partition passes do not apply), c = 12: 2048 buckets"""
    mem = D.members(curve, group, D.REDUCTION_FAMILIES)
    pts = np.stack([w for m in mem for w in (m.P, m.Q)])
    table_mode(monkeypatch, c)
    set_knobs(monkeypatch, dict(pair=0, irr=0, tmin=1, sort="part" if c == 12 else "atomic"))
    bs = gpu.BaseSet(curve, group, pts)
    bad = []
    try:
        for i, m in enumerate(mem):
            for bit in range(c - 1):
                ints = D.reduction_scalars(len(mem), i, bit, c)
                got = gpu.point_to_affine(curve, group, bs.msm(S.wire(curve, ints)))
                want = O.msm(curve, group, pts[2 * i:2 * i + 2], S.wire(curve, ints[2 * i:2 * i + 2]))
                if not check_plan(gpu, c, 1):
                    bad.append((m.name, bit, "the library ran another plan", gpu.msm_last_plan()))
                elif not np.array_equal(got, want):
                    bad.append((m.name, bit))
    finally:
        bs.close()
    assert not bad, f"curve {curve}, G{group}, c = {c}: {len(bad)} of {len(mem) * (c - 1)} (pair, bit) wrong: {bad[:12]}"


@pytest.mark.parametrize("curve,group", GROUPS)
def test_edge_merge_of_designed_points(gpu, monkeypatch, curve, group):
    """lanes of T entries over one bucket of 2T + 1: the lanes' edge pieces are single designed points (T = 1) or hold one"""
    c = M.C_TABLE
    mem = D.members(curve, group, D.REDUCTION_FAMILIES)
    third = D.to_words(curve, group, D.third_point(curve, group))
    pts = np.stack([w for m in mem for w in (m.P, m.Q)] + [third] * (2 * max(D.EDGE_TMINS) - 1))
    table_mode(monkeypatch, c)
    set_knobs(monkeypatch, dict(pair=0, irr=0, tmin=D.EDGE_TMINS[0], sort="part"))
    bs = gpu.BaseSet(curve, group, pts)
    bad = []
    try:
        for T in D.EDGE_TMINS:
            set_knobs(monkeypatch, dict(pair=0, irr=0, tmin=T, sort="part"))
            for i, m in enumerate(mem):
                ints = D.edge_merge_scalars(len(mem), i, T)
                got = gpu.point_to_affine(curve, group, bs.msm(S.wire(curve, ints)))
                want = O.msm(curve, group, np.stack([m.P, m.Q, third]), S.wire(curve, [D.EDGE_BUCKET, D.EDGE_BUCKET, D.EDGE_BUCKET * (2 * T - 1)]))
                if not check_plan(gpu, c, T):
                    bad.append((m.name, T, "the library ran another plan", gpu.msm_last_plan()))
                elif not np.array_equal(got, want):
                    bad.append((m.name, T))
    finally:
        bs.close()
    assert not bad, f"curve {curve}, G{group}: {len(bad)} of {len(mem) * len(D.EDGE_TMINS)} (pair, T) wrong: {bad[:12]}"


# ---- d. the input check ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve,group", GROUPS)
def test_check_points_accepts_every_family(gpu, curve, group):
    for fam, mem in D.families(curve, group).items():
        pts = np.stack([w for m in mem for w in (m.P, m.Q)])
        assert gpu.check_points(curve, group, pts) == (0, 0, 0), fam
