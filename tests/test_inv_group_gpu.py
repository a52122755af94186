"""GPU: the shared inversion of the pairing levels (csrc/fp_inv.hip.h: fp_inv_group, one Bernstein-Yang inversion computed by a group
of 16 lanes, and fp_inv_lanes, Montgomery's trick across those lanes), first on raw limbs, then inside the levels at the lane counts
where the sharing can go wrong.

Raw limbs (op FR_INV_GROUP of mnt753_test_field_raw, groups of 16 consecutive records).  The expectation is the per-lane routine,
op FR_INV (fp_inv), on the same records:
  * k = 1, fp_inv_group itself, once per record of a group with that record's operand in every lane: the LIMBS of fp_inv, bit for bit;
  * k = 0, fp_inv_lanes, every record its own inverse through ONE inversion per group: the same residue.  Its limbs are a product of
    the group's inverse and the sibling products, fp_inv's a product by R'^2: both lie in [0, 2p) and p may lie between them, so the
    two are compared bit for bit after fp_canon (op FR_CANON), the device's own canonical form.
Operands: 0, 1, 2, p - 1, p - 2, (p +- 1) / 2, R' mod p, 2^k for k in {0, 27, 28, 29, 55, 56, 752}, 256 seeded random values in
[0, 2p); placed so that one group holds the same operand in every lane, one is all 1 except one lane, one holds a zero beside
non-zero lanes, and whole waves hold groups of different operands; the list ends in a ragged wave.

The levels: G1 on both curves, window table, c = 12, at most 1024 points, MNT753_MSM_PAIR in {1, 3} x MNT753_MSM_IRR in {0, 2}, with
the buckets chosen by the host model of tests/msm_occupancy.py (a bucket of g entries leaves ceil(g / 2^L) 2^(L - 1) slots to the first
of L levels, every later regular level has half of that, an irregular level ceil(s / 2) per bucket; a level with S slots uses
ceil(S / 8) lanes below the machine's width) so that 1, 15, 16, 17, 63 and 65 lanes are in use
  * in the first level, and
  * in the first level that SHARES its inversion -- the first level of a base field keeps the per-lane inversion (msm_kernels.hip.h):
    the second of three regular levels, or the first irregular level behind one regular level (with MNT753_MSM_IRR = 0 that setting
    shares nothing and must simply stay right);
and two cases in which lane 5 of 16 of the sharing level has a running product of exactly 1 while its neighbours' are not:
  * nothing but odd leftovers -- single points and the stand-ins the level above wrote for cancelled pairs {P, -P};
  * nothing but cancellations INSIDE the sharing level (the pair kind whose denominator is 1): buckets {A, B, -(A + B)}.  Which two
    entries of a bucket meet in a slot of the first level is the sort stage's choice, but here every choice leaves a sum and its
    negative, (A + B, C), (A + C, B) or (B + C, A), to the one slot of the level behind.
After every MSM the plan the library reports must be the plan asked for; the affine result is compared with synth_expected_msm (the
two unit-product cases, whose bases are not the synthetic ones, with the oracle's multi-exp).  An MSM of this size is about 3 ms."""
import collections
import random

import numpy as np
import pytest

import field_raw_ref as F
import msm_occupancy as M
import msm_structured as S
import oracle_lib as O
from test_msm_occupancy_gpu import bases_and_expectation, negate, set_knobs

pytestmark = pytest.mark.gpu

OP_INV, OP_CANON = F.OP_NAMES.index("inv"), F.OP_NAMES.index("canon")
OP_INV_GROUP = 24                     # FR_INV_GROUP of csrc/field_raw_ops.hip.h (test_raw_op_code_is_the_header_s pins it)
G = 16                                # FR_INV_GROUP_LANES = MNT753_PAIR_INV_GROUP


def operands(p, rng):
    edges = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, F.RB % p] + [1 << k for k in (0, 27, 28, 29, 55, 56, 752)]
    rand = [rng.randrange(2 * p) for _ in range(256)]
    vals = []
    vals += [rand[0]] * G                                    # one group, the same operand in every lane
    vals += [1] * 11 + [rand[1]] + [1] * 4                   # all 1 except one lane
    vals += rand[2:9] + [0] + rand[9:15] + [p] + [rand[15]]  # a zero (as 0 and as p) beside non-zero lanes
    vals += edges + [rand[16]]                               # the edges: one group of 15 + 1
    vals += [e + p for e in edges if e + p < 2 * p]          # and their upper representatives in [0, 2p)
    vals += rand                                             # waves of groups with different operands
    vals += edges[:5]                                        # a ragged last wave (and a ragged last group)
    return vals


def records(vals):
    rec = np.zeros((len(vals), 6 * F.NL), dtype=np.uint32)
    for i, v in enumerate(vals):
        rec[i, :F.NL] = F.to_limbs(v)
    return rec


@pytest.fixture(scope="module", params=[0, 1])
def raw(gpu, request):
    """(modulus, records, per-lane fp_inv of the records) -- computed once per modulus, shared read-only"""
    mod = request.param
    vals = operands(F.MODS[mod], random.Random(753 + mod))
    rec = records(vals)
    want = gpu.api.test_field_raw(mod, OP_INV, rec, 0)
    want.setflags(write=False)
    assert len(vals) % 64 != 0 and len(vals) % G != 0
    return mod, vals, rec, want


def test_raw_op_code_is_the_header_s():
    """the literal above is the enumerator of csrc/field_raw_ops.hip.h, which lies behind every op field_raw_ref drives"""
    import os, re
    hdr = os.path.join(O.ROOT, "snark-challenge-prover-reference_amd", "csrc", "field_raw_ops.hip.h")
    m = re.search(r"\bFR_INV_GROUP\s*=\s*(\d+)", open(hdr).read())
    assert m and int(m.group(1)) == OP_INV_GROUP and OP_INV_GROUP >= len(F.OP_NAMES)


def test_group_inversion_limbs(gpu, raw):
    """fp_inv_group on every record's operand (the whole group holds it): the limbs of fp_inv, bit for bit"""
    mod, vals, rec, want = raw
    got = gpu.api.test_field_raw(mod, OP_INV_GROUP, rec, 1)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"modulus {mod}: {bad.size} of {len(vals)} records differ from fp_inv, first at {bad[:8]}"


def test_lanes_inversion_residues(gpu, raw):
    """fp_inv_lanes, a different operand in every lane: in [0, 2p) with normalised limbs, and fp_inv's value bit for bit once both are
    canonical; a zero lane gives zero and leaves its neighbours alone"""
    mod, vals, rec, want = raw
    p = F.MODS[mod]
    got = gpu.api.test_field_raw(mod, OP_INV_GROUP, rec, 0)
    for i in range(len(vals)):
        l = got[i, :F.NL]
        assert F.normalised(l) and F.val_std(l) < 2 * p, f"modulus {mod}, record {i}: outside [0, 2p)"
    canon = lambda out: gpu.api.test_field_raw(mod, OP_CANON, np.hstack([out[:, :F.NL], np.zeros((out.shape[0], 5 * F.NL), dtype=np.uint32)]), 0)[:, :F.NL]
    a, b = canon(got), canon(want)
    bad = np.flatnonzero((a != b).any(axis=1))
    assert bad.size == 0, f"modulus {mod}: {bad.size} of {len(vals)} records differ from fp_inv as residues, first at {bad[:8]}"
    rinv2 = pow(F.RB, 2, p)                                   # x = a R'  ->  a^-1 R' = x^-1 R'^2: an independent look at three records
    for i in (0, 40, len(vals) - 1):
        v = vals[i] % p
        assert F.val_std(a[i]) == (pow(v, -1, p) * rinv2 % p if v else 0)


# ---- the levels ---------------------------------------------------------------------------------------------------------------------------
C_BITS = 12
MIN_B = 8                              # PAIR_MIN_B (msm_host.hpp): slots per lane below the machine's width
LANE_COUNTS = (1, G - 1, G, G + 1, 63, 65)
# entries per bucket, cycled.  first: every bucket is one final slot behind L levels.  sharing: L = 3 the same (the second level has
# half the first one's slots), L = 1 buckets of one or two level-1 slots, one slot each in the irregular level behind
SIZES = {("first", 1): (2, 2, 2, 1), ("first", 3): (2, 3, 5, 8, 1), ("sharing", 1): (3, 1, 1, 3, 1), ("sharing", 3): (2, 3, 5, 8, 1)}


def level_slots(counts, L):
    """(slots of the first of L regular levels, of the second one, of the first irregular level behind them)"""
    first = sum(M.slots(g, L) for g in counts) << (L - 1)
    return first, first >> 1, sum(M.slots(g, L, 1) for g in counts)


def lanes_profile(L, nle, target):
    """buckets 1, 2, ... sized so that the targeted level has S = 8 nle - 4 slots: ceil(S / 8) = nle lanes, the last with half a batch"""
    S_slots = MIN_B * nle - 4
    if target == "first":
        n_buckets = S_slots >> (L - 1)
    else:
        n_buckets = S_slots >> 1 if L == 3 else S_slots
    sizes = SIZES[(target, L)]
    ints, designed = [], collections.Counter()
    for j in range(1, n_buckets + 1):
        M.fill(ints, designed, j, sizes[j % len(sizes)], C_BITS)
    prof = M._profile(ints, designed)
    first, second, irr1 = level_slots(M.designed_counts(prof, C_BITS, True), L)
    at = first if target == "first" else (second if L == 3 else irr1)
    assert len(ints) <= 1024 and at == S_slots and (S_slots + MIN_B - 1) // MIN_B == nle
    return prof


def unit_lane_profile():
    """One regular level and the irregular ones behind it: 124 buckets, one slot each in the first irregular level (slot = bucket rank,
    lane = slot mod 16).  The buckets of lane 5 hold one level-1 slot -- a single point, or {P, -P}, for which level 1 writes its stand-in
    -- so every slot of that lane is an odd leftover; every other bucket holds three different points, an addition in both levels"""
    ints, recipe, designed = [], [], collections.Counter()
    for j in range(1, 125):
        slot = j - 1
        if slot % G == 5:
            items = ["new", ("neg", 0)] if (slot // G) % 2 == 0 else ["new"]
        else:
            items = ["new", "new", "new"]
        first = len(recipe)
        for it in items:
            recipe.append(("synth",) if it == "new" else (it[0], first + it[1]))
            ints.append(j)
        designed[(0, j)] += len(items)
    prof = M.Profile(ints, recipe, dict(designed))
    assert level_slots(M.designed_counts(prof, C_BITS, True), 1)[2] == 124 and len(ints) <= 1024
    return prof


def cancelling_lane_profile():
    """As unit_lane_profile, but the buckets of lane 5 hold three points that sum to the identity (the third base is replaced by
    -(A + B) in cancelling_bases): an addition in level 1 beside a single point, and their cancellation in the sharing level"""
    ints, designed, triples = [], collections.Counter(), []
    for j in range(1, 125):
        if (j - 1) % G == 5:
            triples.append(len(ints))
        ints += [j] * 3
        designed[(0, j)] += 3
    prof = M._profile(ints, designed)
    assert level_slots(M.designed_counts(prof, C_BITS, True), 1)[2] == 124 and len(ints) <= 1024
    return prof, triples


def cancelling_bases(gpu, curve, prof, triples):
    pts, sc, _ = bases_and_expectation(gpu, curve, 1, prof)
    pts = pts.copy()
    ones = S.wire(curve, [1, 1, 1])
    for i in triples:
        pts[i + 2] = negate(curve, 1, O.msm(curve, 1, pts[i:i + 2], ones[:2]))
        assert not O.msm(curve, 1, pts[i:i + 3], ones).any()       # A + B + C is the identity
    want = O.msm(curve, 1, pts, sc)
    assert want.any()
    return pts, sc, want


def run_levels(gpu, monkeypatch, curve, prof, pairs, data=None):
    monkeypatch.setenv("MNT753_MSM_PRECOMP", "1")
    monkeypatch.setenv("MNT753_MSM_TABLE_BITS", str(C_BITS))
    pts, sc, want = data or bases_and_expectation(gpu, curve, 1, prof)
    n = len(prof.ints)
    # a PAIR 6 setting first: it sizes the base set's level buffers so that two irregular levels behind one regular level fit at any n
    # (tests/msm_occupancy.py, run_order); an irregular level without room is dropped, and the plan check below would say so
    knobs = M.run_order(M.knob_product(pairs, (0, 2), (1,), sort="part") + [dict(pair=6, irr=0, tmin=1, sort="part")])
    set_knobs(monkeypatch, knobs[0])
    bs = gpu.BaseSet(curve, 1, pts)
    bad = []
    try:
        for knob in knobs:
            set_knobs(monkeypatch, knob)
            got = gpu.point_to_affine(curve, 1, bs.msm(sc))
            plan = gpu.msm_last_plan()
            asked = dict(window_table=True, window_bits=C_BITS, windows=S.windows(C_BITS), entries_per_lane=M.plan_T(n, C_BITS, 1, 1),
                         pair_levels=knob["pair"], irr_levels=knob["irr"])
            if plan != asked:
                bad.append((knob, "the library ran another plan", plan))
            elif not np.array_equal(got, want):
                bad.append((knob, "wrong group element"))
    finally:
        bs.close()
    assert not bad, f"curve {curve}, n = {n}: {len(bad)} of {len(knobs)} settings fail: {bad}"


@pytest.mark.parametrize("nle", LANE_COUNTS)
@pytest.mark.parametrize("target", ["first", "sharing"])
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("curve", [0, 1])
def test_levels_at_lane_counts(gpu, monkeypatch, curve, L, target, nle):
    """nle lanes in use in the first of L levels, or in the first level that shares its inversion (the other lanes of its last wave
    hold 1 and take part like any other), with and without two irregular levels behind"""
    run_levels(gpu, monkeypatch, curve, lanes_profile(L, nle, target), (L,))


@pytest.mark.parametrize("curve", [0, 1])
def test_lane_with_unit_running_product(gpu, monkeypatch, curve):
    """a lane of the sharing level whose whole batch is odd leftovers, between lanes that add"""
    run_levels(gpu, monkeypatch, curve, unit_lane_profile(), (1,))


@pytest.mark.parametrize("curve", [0, 1])
def test_lane_of_cancellations_in_the_sharing_level(gpu, monkeypatch, curve):
    """a lane of the sharing level whose whole batch cancels there (denominator 1 in every slot), between lanes that add"""
    prof, triples = cancelling_lane_profile()
    run_levels(gpu, monkeypatch, curve, prof, (1,), cancelling_bases(gpu, curve, prof, triples))
