"""The designed points of tests/designed_points.py, checked without a GPU: every member is a pair of different points on its curve,
every family has all of its members and the property it was built for, the low-limb collisions hold on the project's own primitives
(the host twin of csrc/field_raw_ops.hip.h: from_wire, sub_raw, raw_maybe_zero say "maybe zero"; sub, is_zero say "not zero"), and the
expectations tests/test_designed_points_gpu.py takes from the oracle are pinned a second time to tools/pyref.py."""
import numpy as np
import pytest

import designed_points as D
import field_raw_ref as F
import msm_occupancy as M
import msm_structured as S
import oracle_lib as O
import validate_ref as V

GROUPS = [(0, 1), (1, 1), (0, 2), (1, 2)]


@pytest.fixture(scope="module")
def host_twin(tmp_path_factory):
    return F.build_host_twin(tmp_path_factory.mktemp("field_raw_host"))


# ---- well-formedness, counts ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve,group", GROUPS)
def test_members_are_pairs_of_different_points_on_the_curve(curve, group):
    cv = D.CURVES[curve]
    names = set()
    for m, (name, P, Q) in zip(D.members(curve, group), D.members_points(curve, group)):
        assert m.name == name and name not in names
        names.add(name)
        for w, pt in ((m.P, P), (m.Q, Q)):
            assert V.point_verdict(curve, group, w) == V.OK, name
            assert not cv.f_is_zero(pt[1]), name
            assert D.from_words(curve, group, w) == pt, name           # the codec round trip
        assert P != Q, name                                             # different points
        assert (P == cv.neg(Q)) == name.startswith("opposite/"), name    # a point and its negative in that family only


@pytest.mark.parametrize("curve,group", GROUPS)
def test_every_family_has_all_of_its_members(curve, group):
    fams = D.families(curve, group)
    assert {k: len(v) for k, v in fams.items()} == D.COUNTS[(curve, group)]
    total = sum(len(v) for v in fams.values())
    assert total == D.TOTALS[(curve, group)] == {(0, 1): 76, (1, 1): 76, (0, 2): 39, (1, 2): 62}[(curve, group)]
    assert total % 64 and all(len(v) % 64 for v in fams.values())       # ragged on purpose


# ---- the square roots -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve,group", GROUPS)
def test_square_roots(curve, group):
    cv, deg = D.CURVES[curve], D.degree(curve, group)
    squares = 0
    for k in range(2, 14):
        a = D.f_embed(cv, k, deg, k + 1)
        r = D.f_sqrt(curve, a)
        euler = D.f_pow(cv, a, (cv.q ** deg - 1) // 2) == cv.f_one(a)
        assert (r is not None) == euler
        if r is not None:
            assert cv.f_mul(r, r) == a
            squares += 1
        sq = cv.f_mul(a, a)
        assert D.f_sqrt(curve, sq) in (a, cv.f_neg(a))
    assert 0 < squares < 12
    G = cv.gen(group)
    assert D.lift(curve, group, G[0]) in (G, cv.neg(G))


# ---- the properties ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve,group", GROUPS)
def test_same_y(curve, group):
    cv, h = D.CURVES[curve], O.aff_words(curve, group) // 2
    for tri in D.same_y_triples(curve, group):
        assert len({p[0] for p in tri}) == 3 and len({p[1] for p in tri}) == 1
        assert cv.add(tri[0], tri[1], group) == cv.neg(tri[2])           # three points of one line: P1 + P2 = -P3
    mem = D.families(curve, group)["same_y"]
    for m, (name, P, Q) in zip(mem, D.families_points(curve, group)["same_y"]):
        assert not np.array_equal(m.P[:h], m.Q[:h]), name
        if "+" in name:
            assert np.array_equal(m.P[h:], m.Q[h:]), name                 # equal y words: num = 0 under equal sign flags
        else:
            assert cv.f_is_zero(cv.f_add(P[1], Q[1])), name               # y2 = -y1: num = 0 under differing sign flags
    assert sum("+" in m.name for m in mem) == sum("-" in m.name.split("/")[-1] for m in mem) == 12


@pytest.mark.parametrize("curve", [0, 1])
def test_partial_x(curve):
    cv = D.CURVES[curve]
    seen = set()
    for name, P, Q in D.families_points(curve, 2)["partial_x"]:
        eq = D.equal_components(P[0], Q[0])
        assert name.split("/")[1] == "eq" + "".join(str(i) for i in sorted(eq)), name      # exactly the subset the name says
        assert 0 < len(eq) < cv.deg
        assert cv.gen(2) in (P, Q)
        seen.add((eq, name.split("/")[2]))
    assert len(seen) == 2 * ((1 << cv.deg) - 2)                             # every proper non-empty subset, both orders


@pytest.mark.parametrize("curve", [0, 1])
def test_sparse_x(curve):
    cv = D.CURVES[curve]
    pts = D.sparse_points(curve)
    zeros = sorted(sum(c == 0 for c in pt[0]) for _, pt in pts)
    assert zeros == ([1, 1, 1] if cv.deg == 2 else [1, 1, 1, 2, 2, 2])
    assert sum(all(c == 0 for c in pt[0][1:]) for _, pt in pts) >= 1        # x in the base field
    assert len({pt[0] for _, pt in pts}) == len(pts)
    for nz, pt in pts:
        assert [i for i, c in enumerate(pt[0]) if c] == [int(ch) for ch in nz]


def _limb_diff(curve, x1, x2):
    return [F.s32(b) - F.s32(a) for a, b in zip(D.stored_limbs(curve, x1), D.stored_limbs(curve, x2))]


@pytest.mark.parametrize("curve", [0, 1])
def test_neighbour_x(curve):
    fam = {name: (P, Q) for name, P, Q in D.families_points(curve, 1)["neighbour_x"]}
    for kind, low, deltas in D.NEIGHBOUR_STORED:
        for d in deltas:
            P, Q = fam[f"neighbour_x/{kind}/{d:+d}/fwd"]
            assert fam[f"neighbour_x/{kind}/{d:+d}/rev"] == (Q, P)
            assert D.stored(curve, Q[0]) - D.stored(curve, P[0]) == d
            diff = _limb_diff(curve, P[0], Q[0])
            if low is not None:
                assert D.stored_limbs(curve, P[0])[0] == low
                # a carry / borrow into limb 1: limbs of opposite sign in the limb-wise difference
                assert diff[1] == (1 if d > 0 else -1) and diff[0] == d - (diff[1] << F.LB) and diff[0] * diff[1] < 0 and not any(diff[2:])
            else:
                assert diff[0] == d and not any(diff[1:])
    for kind, _ in D.NEIGHBOUR_CANONICAL:
        P, Q = fam[f"neighbour_x/canonical_{kind}/fwd"]
        assert Q[0] - P[0] == 1


@pytest.mark.parametrize("curve", [0, 1])
def test_edge_x(curve):
    q = D.CURVES[curve].q
    pts = D.edge_points(curve)
    assert len({p[0] for p in pts.values()}) == len(pts) == 13
    for name, space, target, step in D.edge_targets(curve):
        x = pts[name][0]
        v = x if space == "x" else D.stored(curve, x) % q
        k, rem = divmod((v - target) % q if step > 0 else (target - v) % q, abs(step))
        assert rem == 0 and k < D.MAX_CANDIDATES, name                       # the nearest: within the walk from its target
    lim = D.stored_limbs(curve, pts["X=limbmax"][0])
    assert all(l == F.MASK for l in lim[:26])
    assert D.stored_limbs(curve, pts["X=2^28-1"][0])[0] == F.MASK and D.stored_limbs(curve, pts["X=2^28"][0])[0] == 0
    for lo, hi in D.EDGE_SMALL_LARGE:                                         # small with large: a stored difference near +-q
        if lo.startswith("X"):
            gap = q - (D.stored(curve, pts[hi][0]) - D.stored(curve, pts[lo][0]))
            assert 0 < gap < 1 << (F.LB * 26 + 8), (lo, hi)                    # q is 2^753: within 2^-17 q of q
        else:
            assert 0 < q - (pts[hi][0] - pts[lo][0]) < 2 * D.MAX_CANDIDATES, (lo, hi)


# ---- low_limb against the project's own primitives -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", [0, 1])
def test_low_limb_on_the_host_twin(host_twin, curve):
    mem = D.families_points(curve, 1)["low_limb"]
    maybe, zero, l1, l2 = D.low_limb_chain(host_twin, curve, [(P[0], Q[0]) for _, P, Q in mem])
    seen = set()
    for i, (name, P, Q) in enumerate(mem):
        assert [int(w) for w in l1[i]] == D.stored_limbs(curve, P[0]), name   # the model of the stored form, representative included
        assert [int(w) for w in l2[i]] == D.stored_limbs(curve, Q[0]), name
        assert maybe[i] == 1 and zero[i] == 0, name                           # the quick test fires, the exact one settles it
        _, anchor, pat, order = name.split("/")
        want = pat if order == "fwd" else {"0": "0", "+p0": "-p0", "-p0": "+p0"}[pat]
        assert D.low_limb_pattern(curve, P[0], Q[0]) == want, name
        seen.add((anchor, order, want))
    assert seen == {(a, o, p) for a in ("gen", "lift") for o in ("fwd", "rev") for p in D.LOW_LIMB_PATTERNS}
    # The other G1 pairs: the quick test fires exactly where the model of the stored limbs shows one of the three patterns, and the exact
    # test settles every one as "not zero".  On MNT4753 none fires.  On MNT6753 p_0 = 1, so a stored difference of +-1 IS the pattern
    # +-p_0: the +-1 members of neighbour_x and the pair of stored residues next to 0 and q - 1 (difference -+1 mod q) fire as well.
    rest = D.members_points(curve, 1, ("same_y", "neighbour_x", "edge_x"))        # (opposite: x2 - x1 IS zero)
    maybe, zero, _, _ = D.low_limb_chain(host_twin, curve, [(P[0], Q[0]) for _, P, Q in rest])
    assert not zero.any()
    fired = [name for (name, _, _), f in zip(rest, maybe) if f]
    assert fired == [name for name, P, Q in rest if D.low_limb_pattern(curve, P[0], Q[0]) is not None]
    assert fired == ([] if curve == 0 else OTHER_QUICK_HITS_MNT6753)


OTHER_QUICK_HITS_MNT6753 = ["neighbour_x/carry/+1/fwd", "neighbour_x/carry/+1/rev", "neighbour_x/borrow/-1/fwd", "neighbour_x/borrow/-1/rev",
                            "neighbour_x/plain/+1/fwd", "neighbour_x/plain/+1/rev", "edge_x/X=0/X=q-1", "edge_x/X=q-1/X=0"]


# ---- expectations pinned twice ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve,group", GROUPS)
def test_oracle_addition_equals_pyref(curve, group):
    cv = D.CURVES[curve]
    for m, (name, P, Q) in zip(D.members(curve, group), D.members_points(curve, group)):
        want = D.to_words(curve, group, cv.add(P, Q, group))
        assert np.array_equal(O.point_op(curve, group, 0, m.P, m.Q), want), name
    for pt in D.distinct_points(curve, group):
        assert np.array_equal(O.point_op(curve, group, 1, D.to_words(curve, group, pt)), D.to_words(curve, group, cv.add(pt, pt, group)))


CASES = [(curve, group, cs) for curve, group in GROUPS for cs in D.pair_bucket_cases(curve, group)]


@pytest.mark.parametrize("curve,group,cs", CASES, ids=[f"{c}-G{g}-{cs.name}" for c, g, cs in CASES])
def test_pair_bucket_input(curve, group, cs):
    """every pair sits in a bucket of its own with the sign flags designed, the carries in bucket 1; the oracle's multi-exp equals
    pyref's; and the settings run as asked (msm_occupancy.replay)"""
    cv = D.CURVES[curve]
    pts, ints, keys = cs.build(curve)
    mem = D.members(curve, group)
    assert len(ints) == len(pts) == 4 * len(mem) and len(keys) == 2 * len(mem)
    nb = 1 << (cs.c - 1)
    got = {}
    for k, s in enumerate(ints):
        for w, d in enumerate(S.booth(s, cs.c)):
            if d:
                got.setdefault((0 if cs.table else w * nb) + abs(d) - 1, []).append((k, d < 0, w))
    carries = 0
    for key, entries in got.items():
        if key in keys:
            i, flagged = keys[key]
            assert sorted((k % 2, neg_) for k, neg_, _ in entries) == [(0, False), (1, flagged)]
            assert all(np.array_equal(pts[k], mem[i].Q if k % 2 else mem[i].P) for k, _, _ in entries)
            assert all(w == (0 if cs.table else key // nb) for _, _, w in entries)
        else:
            assert key % nb == 0 and all(not neg_ and k % 2 for k, neg_, _ in entries)     # bucket 1: the carries of the flagged copy
            carries += len(entries)
    assert carries == len(mem) and set(keys) <= set(got)
    want = cv.msm(ints, [D.from_words(curve, group, p) for p in pts], group)
    assert want is not None
    assert np.array_equal(O.msm(curve, group, pts, S.wire(curve, ints)), D.to_words(curve, group, want))
    lanes = M.lanes_per_point(curve, group)
    for knob, by_partition, irr_run in M.replay(cs, len(ints), lanes):
        assert M.plan_T(len(ints), cs.c, lanes, knob["tmin"]) == knob["tmin"]
        assert irr_run == knob["irr"], knob
        if cs.table and knob["sort"] != "atomic":
            assert by_partition, knob


@pytest.mark.parametrize("curve,group", GROUPS)
def test_reduction_keys(curve, group):
    for c in (8, 12):
        n = len(D.members(curve, group, D.REDUCTION_FAMILIES))
        for i in range(n):
            for bit in range(c - 1):
                kp, kq = D.reduction_keys(i, bit, c)
                assert kp ^ kq == 1 << bit and 0 <= kp < (1 << (c - 1)) - 1 and 0 <= kq < (1 << (c - 1)) - 1
                ints = D.reduction_scalars(n, i, bit, c)
                assert [S.booth(s, c)[0] for s in ints if s] == [kp + 1, kq + 1] and all(not any(S.booth(s, c)[1:]) for s in ints)
