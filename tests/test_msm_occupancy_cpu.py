"""CPU: the occupancy profiles of tests/msm_occupancy.py do what they are built for, and the host model says that the cases
tests/test_msm_occupancy_gpu.py runs -- the one list msm_occupancy.all_cases() -- drive the bucket stages through every event the
model knows.  The conditions are requirements on the profiles, not measurements: where one fails, the profile changes.

Also pinned here: the plan the model restates (T = MNT753_MSM_TMIN at every size the GPU file uses), the stand-in point of the
batched-affine levels as the test library hands it out, and the expectations the GPU file compares with (the discrete logs of the
synthetic bases against the oracle's multi-exp, on the staircase and on the replaced bases of `collisions`)."""
import numpy as np
import pytest

import msm_occupancy as M
import msm_structured as S
import oracle_lib as O
import pyref
import validate_ref as V

CASES = M.all_cases()
CASE_IDS = [f"curve{curve}-g{group}-{cs.name}" for curve, group, cs in CASES]
GROUPS = [(0, 1), (0, 2), (1, 1), (1, 2)]
_PROFILES = {}


def profile(curve, group, cs):
    key = (curve, group, cs.name, cs.c, cs.table)
    if key not in _PROFILES:
        _PROFILES[key] = cs.build(curve)
    return _PROFILES[key]


# ---- occupancy --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve,group,cs", CASES, ids=CASE_IDS)
def test_profiles_give_the_designed_counts(curve, group, cs):
    """the reference recoding of every scalar, at the width and in the mode the GPU file runs the case, against the counts the profile
    was built for; every scalar is below r and the base recipe names earlier bases only"""
    prof = profile(curve, group, cs)
    r = S.modulus(curve)
    assert prof.ints and all(0 <= s < r for s in prof.ints)
    assert M.occupancy(prof.ints, cs.c, cs.table) == M.designed_counts(prof, cs.c, cs.table)
    if prof.recipe is not None:
        assert len(prof.recipe) == len(prof.ints)
        for i, it in enumerate(prof.recipe):
            assert it[0] in ("synth", "copy", "neg", "gen")
            if it[0] in ("copy", "neg"):
                assert it[1] < i and prof.recipe[it[1]] == ("synth",)


def test_the_designs_are_the_ones_the_profiles_are_named_for():
    c, nb = M.C_TABLE, 1 << (M.C_TABLE - 1)
    for form in ("wide", "tall"):
        p = M.staircase(0, c, form)
        assert M.designed_counts(p, c, True)[:41] == list(range(1, 41)) + [0] and len(p.ints) == (820 if form == "wide" else 40)
    tall = M.staircase(0, c, "tall")
    assert {w for (w, j) in tall.designed if j == 40} == set(range(40))              # rows of 40 table levels in one bucket
    p = M.powers(0, c)
    assert len(p.ints) == 762
    assert M.designed_counts(p, c, True)[:22] == [g for k in range(1, 8) for g in (2 ** k - 1, 2 ** k, 2 ** k + 1)] + [0]
    for T, phase in ((3, 0), (8, 7), (64, 1)):
        got = M.designed_counts(M.aligned(0, c, T, phase, "tall" if T > 8 else "wide"), c, True)
        assert got[:26] == [phase] + [T * q for _ in range(8) for q in (1, 2, 3)] + [0]
    # ends: the extreme digit is the last key of the set, negated, and its carry +1 is an entry of the window above
    p = M.ends(0, c)
    assert S.booth(1 << (c - 1), c)[:3] == [-nb, 1, 0]
    t = M.occupancy(p.ints, c, True)
    assert (t[0], t[nb // 2 - 1], t[nb - 1], sum(t)) == (74, 1, 37, 112)
    c7, nb7 = M.C_NO_TABLE, 1 << (M.C_NO_TABLE - 1)
    s = M.occupancy(M.ends(0, c7).ints, c7, False)
    assert (s[0], s[nb7 // 2 - 1], s[nb7 - 1], s[nb7], sum(s)) == (37, 1, 37, 37, 112)
    # without the table the second staircase sits in set FAR_WINDOW alone
    far = M.occupancy(M.staircase(0, c7, "wide", top=M.NO_TABLE_STEPS, window=M.FAR_WINDOW).ints, c7, False)
    assert far[M.FAR_WINDOW * nb7:M.FAR_WINDOW * nb7 + 35] == list(range(1, 35)) + [0] and sum(far) == 595
    # full_set: 128 keys, sizes 0 .. 7 all present, one run of 16 empty keys, the last key holds the extreme digits
    f = M.occupancy(M.full_set(0).ints, 8, True)
    assert len(f) == 128 and set(f[8:56]) == set(range(8)) and f[56:72] == [0] * 16 and f[55] and f[72] and f[127] == 3
    # nibbles: 15 adjacent buckets near n / 16, nothing above
    nib = M.occupancy(M.nibbles(0, c, 1024).ints, c, True)
    assert all(32 <= g <= 96 for g in nib[:15]) and not any(nib[15:])
    # collisions: at most about 120 bases
    assert len(M.collisions(0, c).ints) <= 120


# ---- coverage: what the GPU file's runs make the bucket stages do ---------------------------------------------------------------------------
def views():
    """[(case name, knob, list the accumulate walks, its T)] and [(case name, bucket sizes, L)] over everything the GPU file runs"""
    acc, trees = [], []
    for curve, group, cs in CASES:
        prof = profile(curve, group, cs)
        counts = M.occupancy(prof.ints, cs.c, cs.table)
        seen_L = set()
        for knob in cs.knobs:
            T = M.plan_T(len(prof.ints), cs.c, M.lanes_per_point(curve, group), knob["tmin"])
            acc.append((cs.name, knob) + M.accumulate_view(counts, knob, T))
            if knob["pair"] and knob["pair"] not in seen_L:
                seen_L.add(knob["pair"])
                trees.append((cs.name, counts, knob["pair"]))
    return acc, trees


def test_every_lane_event_occurs_at_both_forms_of_the_accumulate():
    """each kind of lane_events at least once in front of the plain accumulate (PAIR = 0) and once behind levels (the BLOCKED form)"""
    acc, _ = views()
    for blocked in (False, True):
        total = dict.fromkeys(M.LANE_EVENTS, 0)
        for name, knob, sizes, T in acc:
            if bool(knob["pair"]) == blocked:
                for k, v in M.lane_events(sizes, T).items():
                    total[k] += v
        assert all(total.values()), (blocked, total)


def test_aligned_puts_every_bucket_end_on_a_lane_end_or_none():
    """aligned(T, .) in front of the plain accumulate at TMIN = T, aligned(8 * 2^L, .) behind L regular levels (irregular levels halve
    the slots again: no multiples of 8 any more, a case like any other)"""
    acc, _ = views()
    checked = 0
    for name, knob, sizes, T in acc:
        if not ((name.startswith("aligned_T") and knob["pair"] == 0) or (name.startswith("aligned_blocked") and knob["irr"] == 0 and f"_L{knob['pair']}_" in name)):
            continue
        ev = M.lane_events(sizes, T)
        buckets = sum(1 for g in sizes if g)
        if name.endswith("_p0"):
            assert buckets == M.ALIGNED_BUCKETS and ev["end_on_lane_end"] == buckets, (name, knob, ev)
        else:
            assert buckets == M.ALIGNED_BUCKETS + 1 and ev["end_on_lane_end"] == 0, (name, knob, ev)
        assert ev["spans_3_lanes"] >= 8                       # the buckets of 3 T entries
        checked += 1
    assert checked == 2 * (9 + 8 * len(M.TMINS) + 3 + 2 * 2)   # per curve: G1 plain, G1 blocked, G2 plain, G2 blocked


def test_every_residue_and_slot_kind_of_the_regular_tree_occurs():
    """g mod 2^L in {0, 1, 2^L - 1} for every L the GPU file runs; a SINGLE slot at every level up to 3; a group that is all padding"""
    _, trees = views()
    residues = {L: set() for L in M.PAIRS if L}
    single = {L: [0] * L for L in residues}
    empty = {L: [0] * L for L in residues}
    for name, counts, L in trees:
        ev = M.tree_events(counts, L)
        residues[L] |= ev["residues"]
        for l, lv in enumerate(ev["levels"]):
            single[L][l] += lv["single"]
            empty[L][l] += lv["empty"]
    assert set(residues) == {1, 2, 3, 6}
    for L in residues:
        assert {0, 1, (1 << L) - 1} <= residues[L], (L, sorted(residues[L]))
        assert all(single[L][:3]), (L, single[L])
        if L > 1:
            # an EMPTY slot at every level below the top one: 2^l entries of padding in a row (the top level has none: a bucket gets
            # ceil(g / 2^L) final slots, each with an entry under it)
            assert all(empty[L][:-1]) and not empty[L][-1], (L, empty[L])
    # and the irregular levels meet buckets with an odd and an even number of slots, and with one slot
    left = {M.slots(g, L) for name, counts, L in trees for g in counts if g}
    assert 1 in left and any(s % 2 for s in left if s > 1) and any(s % 2 == 0 for s in left)


def test_model_of_slots_and_events_on_small_lists():
    assert [M.slots(g, 3) for g in (1, 8, 9, 16, 17)] == [1, 1, 2, 2, 3]
    assert [M.slots(g, 1, 2) for g in (1, 2, 3, 8, 9)] == [1, 1, 1, 1, 2]
    # T = 4 over sizes 4 | 0 | 0 | 9 | 1 | 1 | 1 | 3: lanes [4] [9 9 9 9] [9 9 9 9] [9 1 1 1] [3 3 3]
    ev = M.lane_events([4, 0, 0, 9, 1, 1, 1, 3], 4)
    assert ev == dict(end_on_lane_end=2, spans_3_lanes=1, two_whole_buckets=1, single_run_lane=4, starts_behind_empty_keys=1, skips_empty_keys=0)
    assert M.lane_events([2, 0, 3], 4)["skips_empty_keys"] == 1
    t = M.tree_events([1, 5, 8], 3)
    assert t["residues"] == {1, 5, 0}
    assert t["levels"] == [dict(pair=6, single=2, empty=4), dict(pair=3, single=2, empty=1), dict(pair=2, single=1, empty=0)]


# ---- the plan -------------------------------------------------------------------------------------------------------------------------------
def test_plan_gives_tmin_at_every_size_the_gpu_file_uses():
    assert M.plan_T(1024, 12, 1, 1) == 1 and M.plan_T(1041, 12, 1, 1) == 2          # 63 * 1041 > 65536
    assert M.plan_T(1 << 20, 19, 1, 8) == 320 and M.plan_T(1 << 20, 12, 1, 8) == 504  # two rounds from 2^23 entries on
    assert M.plan_T(512, 12, 2, 1) == 1 and M.plan_T(336, 12, 3, 1) == 1 and M.plan_T(342, 12, 3, 1) == 2
    for curve, group, cs in CASES:
        n = len(profile(curve, group, cs).ints)
        for knob in cs.knobs:
            assert M.plan_T(n, cs.c, M.lanes_per_point(curve, group), knob["tmin"]) == knob["tmin"], (curve, group, cs.name, n)


def test_state_the_plan_does_not_report():
    """The library does not report which sort stage ran, and it drops irregular levels that do not fit its level buffers (the GPU file
    sees that in the reported irr_levels, after the fact).  Restated from ensure_ws / ensure_pair_ws / pair_and_accumulate: in the order
    every case runs its settings, each part / generic setting finds the partition buffers and each setting has room for every
    irregular level it asks for -- and the order matters: the settings as first written (atomic ahead of generic, PAIR 0 first) fail both."""
    for curve, group, cs in CASES:
        n = len(profile(curve, group, cs).ints)
        assert cs.knobs == M.run_order(cs.knobs)
        for knob, by_partition, irr_run in M.replay(cs, n, M.lanes_per_point(curve, group)):
            assert by_partition == (knob["sort"] != "atomic"), (curve, group, cs.name, knob)
            assert irr_run == knob["irr"], (curve, group, cs.name, n, knob, irr_run)
    assert M.partition_fits(12, True) and not M.partition_fits(8, True)
    # the model sees what the order is for: staircase_tall (n = 40) with PAIR 0 first and the extras as the issue lists them
    cs = next(c for c in M.g1_cases() if c.name == "staircase_tall")
    naive = cs._replace(knobs=M.G1_KNOBS + M.G1_EXTRAS)
    got = M.replay(naive, 40, 1)
    assert any(k["sort"] == "generic" and not part for k, part, _ in got)
    assert any(k["pair"] == 1 and k["irr"] == 3 and run == 1 for k, _, run in got)
    assert M.irr_levels_run(40, 12, True, 1, 3, M.pair_cap1(40, 12, True, 1), 2048) == 1      # need 3643 slots, room 2284


# ---- the stand-in point ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve,group", GROUPS)
def test_generator_hook(pkg, curve, group):
    """mnt753_test_generator: on its curve, not the identity, and word for word the generator the library's constants were generated
    from (tools/mnt753_params.py through tools/pyref.py) -- which is also the G the discrete logs of the synthetic bases refer to"""
    g = pkg.api.test_generator(curve, group)
    assert g.shape == (pkg.affine_words(curve, group),)
    assert g[g.size // 2:].any()                                                  # y != 0: not the identity
    assert V.point_verdict(curve, group, g) == V.OK
    cv = pyref.Curve(curve)
    want = np.array(cv.affine_to_words(cv.gen(group), group), dtype=np.uint64).reshape(-1)
    assert g.tobytes() == want.tobytes()
    # e G is what synth_expected_msm says of the scalar 1 on base 0 = e_0 G, and base 0 is that point
    one = S.wire(curve, [1])
    base0 = pkg.synth_points(curve, group, 77, 1, threads=1)[0]
    assert np.array_equal(pkg.point_to_affine(curve, group, pkg.synth_expected_msm(curve, group, 77, one)), base0)
    assert np.array_equal(O.point_op(curve, group, 2, O.point_op(curve, group, 0, g, base0), base0), g)   # (G + P) - P through the oracle


# ---- the expectations the GPU file uses ---------------------------------------------------------------------------------------------------
def negate(curve, group, p):
    h = p.size // 2
    out = p.copy()
    out[h:] = O.neg_fq(curve, p[h:]) if group == 1 else O.ext_op(curve, 5, p[h:])
    return out


def bases_of(pkg, curve, group, seed, prof):
    synth = pkg.synth_points(curve, group, seed, len(prof.ints), threads=2)
    return M.apply_recipe(prof.recipe, synth, pkg.api.test_generator(curve, group), lambda p: negate(curve, group, p))


@pytest.mark.parametrize("curve", [0, 1])
def test_staircase_expectation_is_the_oracles(pkg, curve):
    prof = M.staircase(curve, M.C_TABLE, "wide")
    sc = S.wire(curve, prof.ints)
    want = pkg.point_to_affine(curve, 1, pkg.synth_expected_msm(curve, 1, 9600 + curve, sc))
    assert want.any()
    assert np.array_equal(O.msm(curve, 1, bases_of(pkg, curve, 1, 9600 + curve, prof), sc), want)


@pytest.mark.parametrize("curve,group", GROUPS)
def test_collisions_expectation_is_the_oracles(pkg, curve, group):
    """replaced bases: the oracle's multi-exp over the points as they are against the discrete logs with every copy's and negative's
    scalar moved onto its original base, plus the coefficient of G"""
    seed = 9610 + 2 * curve + group
    prof = M.collisions(curve, M.C_TABLE)
    pts = bases_of(pkg, curve, group, seed, prof)
    for i, it in enumerate(prof.recipe):                     # the recipe did what it says
        if it[0] == "neg":
            assert np.array_equal(pts[i][:pts[i].size // 2], pts[it[1]][:pts[i].size // 2]) and not np.array_equal(pts[i], pts[it[1]])
            assert not O.point_op(curve, group, 0, pts[i], pts[it[1]])[pts[i].size // 2:].any()       # P + (-P) = the identity
    got = O.msm(curve, group, pts, S.wire(curve, prof.ints))
    moved, coeff = M.moved_scalars(curve, prof)
    assert coeff == (11 - 12 + 2 * 13) % S.modulus(curve)                                             # G, -G, 2 G, G - G
    gen = pkg.point_from_affine(curve, group, pkg.api.test_generator(curve, group))
    want = pkg.point_add(curve, group, pkg.synth_expected_msm(curve, group, seed, S.wire(curve, moved)),
                         pkg.point_scale(curve, group, S.wire(curve, [coeff])[0], gen))
    assert got.any() and np.array_equal(got, pkg.point_to_affine(curve, group, want))
