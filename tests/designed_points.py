"""Curve points with DESIGNED coordinates for the group-law kernels (TEST INFRASTRUCTURE, pure Python over tools/pyref.py).

Every other point the suite feeds to a kernel has coordinates that are uniform for practical purposes, so the branches a relation
between coordinates triggers are never taken.  The families here plant those relations.  G1 of both curves has cofactor 1, so any
(x, sqrt(x^3 + a x + b)) is a valid base; the group law and the CPU oracle hold on the whole twist curve, so G2 points off the
subgroup are valid inputs too.  A member is a named tuple (name, P, Q) of affine wire words.

G1 (the stored form of a coordinate is what k_bases_to_internal writes: fp_from_wire's lazy output, modelled exactly by `stored`):
    low_limb     partners of two anchors whose stored x differs from the anchor's but whose limb-0 difference is 0, p_0 or -p_0 mod 2^28:
                 the quick zero test of k_pair_level (fp_raw_maybe_zero) fires and the exact test has to settle it as "not zero"
    same_y       triples (x_1, y), (x_2, y), (x_3, y) on one horizontal line, x_{2,3} = (-x_1 +- sqrt(-3 x_1^2 - 4a)) / 2: lambda = 0 in the
                 affine addition, u = 0 with v != 0 in the projective ones, P_1 + P_2 = -P_3; all ordered pairs (P_i, P_j) and (P_i, -P_j)
    neighbour_x  stored x values that differ by +-1, +-2 -- anchors with low limb 0xFFFFFFF (a carry) or 0 (a borrow), so that the limb-wise
                 difference has limbs of opposite sign --, and canonical x values that differ by 1
    edge_x       points nearest to canonical x in {0, 1, 2, q-2, q-1, (q-1)/2} and to stored residues X' = x R' in {0, 1, 2^28 - 1, 2^28,
                 R' mod q, q - 1, the largest value below q with limbs 0 .. 25 all 0xFFFFFFF}; each with the generator, small with large
G2:
    partial_x    for every proper non-empty subset of the components of x, a partner of the generator equal to it in exactly that subset
    same_y       as above, the quadratic solved in Fq2 / Fq3
    sparse_x     x with one or two zero components and x in the base field, each with the generator and with each other
Both groups:
    opposite     (P, -P) on designed coordinates: v = 0 with u != 0, the other half of every `same = is_zero(u) && is_zero(v)` (an on-curve
                 pair with equal x and different y is a point and its negative, nothing else); the cancellation of the levels and, where
                 the second base carries a negative digit, their doubling -- at x = 0 among others

Sizes: 76 pairs on G1 (71 of the families asked for, and `opposite`), 39 and 62 on G2 -- ragged on purpose, and G1 a dozen above the ~64 the
families were planned for, because every ordered pair of both same_y triples is kept.  With the Z = 1 row and three representatives of
each operand a hook launch of tests/test_designed_points_gpu.py has 7 rows per pair: up to 532 lanes, three workgroups of the one-lane
geometry and up to seven of the three-lane one, each with a ragged tail.

A search for a liftable value walks at most MAX_CANDIDATES candidates from its target in a fixed order and raises LookupError: no member
is ever dropped.  tests/test_designed_points_cpu.py checks every claim made here; tests/test_designed_points_gpu.py runs the families.

Out of scope, on purpose: the levels behind the first (k_pair_level<..., first = false>, regular and irregular) run the same decision
code on the previous level's sums.  The representative and the low limb of those sums cannot be chosen, and the order of entries inside
a bucket is not fixed by the sort stage (tests/msm_occupancy.py), so a designed collision there would hold for one of three orders and
could not be observed.  There is no probabilistic case.
"""
import collections
import functools
import itertools

import numpy as np

import field_raw_ref as FR
import msm_occupancy as M
import msm_structured as S
import pyref

Member = collections.namedtuple("Member", "name P Q")

CURVES = {0: pyref.Curve(0), 1: pyref.Curve(1)}
MAX_CANDIDATES = 64
MASK = FR.MASK
R_WIRE = pyref.R


def field_mod(curve):
    """index of the curve's Fq in field_raw_ref.MODS / the field_raw hooks: Fq of MNT4753 is modulus B"""
    return 1 if curve == 0 else 0


def degree(curve, group):
    return 1 if group == 1 else CURVES[curve].deg


# ---- field helpers over pyref elements (int, or a tuple of ints) ------------------------------------------------------------------------
def f_deg(x):
    return 1 if isinstance(x, int) else len(x)


def f_pow(cv, x, e):
    if isinstance(x, int):
        return pow(x, e, cv.q)
    r = cv.f_one(x)
    for bit in bin(e)[2:]:
        r = cv.f_mul(r, r)
        if bit == "1":
            r = cv.f_mul(r, x)
    return r


def f_embed(cv, v, deg, fill=0):
    """the base-field value v as an element of the degree-`deg` field: (v, fill, 0 ...)"""
    return v % cv.q if deg == 1 else tuple([v % cv.q, fill % cv.q] + [0] * (deg - 2))


def f_scale(cv, x, k):
    """x times the base-field integer k"""
    return x * k % cv.q if isinstance(x, int) else tuple(c * k % cv.q for c in x)


@functools.lru_cache(maxsize=None)
def _two_adic(curve, deg):
    """(s, t, c = z^t for a non-residue z) of the multiplicative group of order q^deg - 1 = 2^s t"""
    cv = CURVES[curve]
    order = cv.q ** deg - 1
    s = (order & -order).bit_length() - 1
    t = order >> s
    one = cv.f_one(f_embed(cv, 1, deg))
    for j in range(2, 2 + MAX_CANDIDATES):
        z = j if deg == 1 else f_embed(cv, j, deg, 1)
        if f_pow(cv, z, order >> 1) != one:
            return s, t, f_pow(cv, z, t)
    raise LookupError("no quadratic non-residue among the first candidates")


def f_sqrt(curve, a):
    """Tonelli-Shanks in Fq, Fq2 or Fq3 (q = 1 mod 4 on both curves; the 2-adicity of q^k - 1 is 15 / 16 on MNT4753 and 30 on MNT6753):
    a square root of a, or None where a is not a square.  Deterministic."""
    cv = CURVES[curve]
    if cv.f_is_zero(a):
        return a
    s, t, c = _two_adic(curve, f_deg(a))
    one = cv.f_one(a)
    w = f_pow(cv, a, (t - 1) >> 1)
    x = cv.f_mul(a, w)            # a^((t + 1) / 2)
    b = cv.f_mul(x, w)            # a^t
    m = s
    while b != one:
        i, b2 = 0, b
        while b2 != one:
            b2 = cv.f_mul(b2, b2)
            i += 1
            if i == m:
                return None       # the order of a^t does not divide 2^(s - 1): not a square
        e = c
        for _ in range(m - i - 1):
            e = cv.f_mul(e, e)
        x = cv.f_mul(x, e)
        c = cv.f_mul(e, e)
        b = cv.f_mul(b, c)
        m = i
    assert cv.f_mul(x, x) == a
    return x


def curve_rhs(curve, group, x):
    cv = CURVES[curve]
    return cv.f_add(cv.f_add(cv.f_mul(cv.f_mul(x, x), x), cv.f_mul(cv.coeff_a(group), x)), cv.coeff_b(group))


def lift(curve, group, x):
    """(x, y) on the curve of `group` with y != 0, or None where x^3 + a x + b is not a square (or is zero)"""
    y = f_sqrt(curve, curve_rhs(curve, group, x))
    if y is None or CURVES[curve].f_is_zero(y):
        return None
    return (x, y)


def first_liftable(curve, group, candidates, accept=lambda pt: True):
    """the first point over the x values of `candidates` (a deterministic walk away from a target) that lifts and is accepted; at most
    MAX_CANDIDATES are tried, then LookupError"""
    for x in itertools.islice(candidates, MAX_CANDIDATES):
        pt = lift(curve, group, x)
        if pt is not None and accept(pt):
            return pt
    raise LookupError(f"curve {curve}, G{group}: no liftable value among {MAX_CANDIDATES} candidates")


# ---- codecs -------------------------------------------------------------------------------------------------------------------------------
def to_words(curve, group, pt):
    return np.array(CURVES[curve].affine_to_words(pt, group), dtype=np.uint64)


def from_words(curve, group, words):
    return CURVES[curve].affine_from_words([int(w) for w in words], group)


def proj_words(curve, group, pt, lam=None):
    """the projective representative (lam x, lam y, lam) of an affine point in wire words (lam = None: Z = 1)"""
    cv = CURVES[curve]
    x, y = pt
    z = cv.f_one(x)
    if lam is not None:
        x, y, z = cv.f_mul(lam, x), cv.f_mul(lam, y), lam
    return np.array(cv.coord_to_words(x) + cv.coord_to_words(y) + cv.coord_to_words(z), dtype=np.uint64)


def neg(curve, pt):
    return CURVES[curve].neg(pt)


# ---- the stored form of a G1 coordinate ---------------------------------------------------------------------------------------------------
def k_in(curve):
    """the constant fp_from_wire multiplies by: wire is x 2^768, the device form x 2^756, one Montgomery product by 2^744 takes off 2^12"""
    return pow(2, 744, CURVES[curve].q)


def wire_int(curve, x):
    return x * R_WIRE % CURVES[curve].q


def stored(curve, x):
    """the exact integer k_bases_to_internal stores for the base-field coordinate x: the Montgomery product of the wire words with
    k_in, representative included (fp_mul's contract, field_raw_ref.check: (a b + m p) / R' with m in [0, R'))"""
    return FR.mont(wire_int(curve, x), k_in(curve), CURVES[curve].q)


def stored_limbs(curve, x):
    return FR.to_limbs(stored(curve, x))


def x_of_residue(curve, X):
    """the coordinate whose stored residue x R' mod q is X"""
    q = CURVES[curve].q
    return X % q * pow(FR.RB, -1, q) % q


def wire_u32(curve, x):
    """the 24 u32 wire words of a base-field coordinate (operand of the field_raw op from_wire)"""
    w = wire_int(curve, x)
    return [(w >> (32 * j)) & 0xFFFFFFFF for j in range(24)]


LOW_LIMB_PATTERNS = ("0", "+p0", "-p0")


def low_limb_pattern(curve, x1, x2):
    """which of the three patterns fp_raw_maybe_zero accepts the limb-wise difference x2 - x1 of the stored forms shows, or None"""
    p0 = CURVES[curve].q & MASK
    t = (stored(curve, x2) - stored(curve, x1)) & MASK
    return {0: "0", p0: "+p0", (-p0) & MASK: "-p0"}.get(t)


def low_limb_chain(hook, curve, pairs):
    """(maybe-zero flags, is-zero flags, stored limbs of x1, of x2) for [(x1, x2)] through from_wire, sub_raw / raw_maybe_zero and sub /
    is_zero of a field_raw hook -- the chain k_pair_level runs on a first-level slot"""
    mod = field_mod(curve)
    n = len(pairs)
    lim = hook(mod, FR.FROM_WIRE, FR.records_array([[wire_u32(curve, x) + [0, 0, 0]] for pr in pairs for x in pr]), 0)[:, :FR.NL]
    l1, l2 = lim[0::2], lim[1::2]
    two = FR.records_array([[list(b), list(a)] for a, b in zip(l1, l2)])      # x2 - x1
    den = hook(mod, FR.SUB_RAW, two, 0)[:, :FR.NL]
    maybe = hook(mod, FR.RAW_MAYBE_ZERO, FR.records_array([[list(d)] for d in den]), 0)[:, 2 * FR.NL]
    du = hook(mod, FR.SUB, two, 0)[:, :FR.NL]
    zero = hook(mod, FR.IS_ZERO, FR.records_array([[list(d)] for d in du]), 0)[:, 2 * FR.NL]
    assert len(maybe) == len(zero) == n
    return maybe, zero, l1, l2


# ---- G1 families --------------------------------------------------------------------------------------------------------------------------
ANCHOR_X = 5          # target of the lifted anchor / of the generic searches


@functools.lru_cache(maxsize=None)
def g1_anchors(curve):
    cv = CURVES[curve]
    return (("gen", cv.gen(1)), ("lift", first_liftable(curve, 1, (ANCHOR_X + k for k in itertools.count()))))


@functools.lru_cache(maxsize=None)
def low_limb(curve):
    """[(name, P, Q)] as points: per anchor and pattern one partner, both orders.  Designed on X' = x R' mod q with the offsets
    {0, +-p0, +-2 p0} + k 2^28; a candidate is kept for the pattern the MODEL of the stored limbs shows."""
    cv = CURVES[curve]
    p0 = cv.q & MASK
    out = []
    for aname, A in g1_anchors(curve):
        XA = stored(curve, A[0]) % cv.q
        cands = (x_of_residue(curve, XA + off + (k << FR.LB)) for k in itertools.count(1) for off in (0, p0, -p0, 2 * p0, -2 * p0))
        found = {}
        for x in itertools.islice(cands, MAX_CANDIDATES):
            pat = low_limb_pattern(curve, A[0], x)
            if pat is None or pat in found or x == A[0]:
                continue
            pt = lift(curve, 1, x)
            if pt is not None:
                found[pat] = pt
            if len(found) == 3:
                break
        if len(found) != 3:
            raise LookupError(f"curve {curve}: low_limb patterns {sorted(found)} only, anchor {aname}")
        for pat in LOW_LIMB_PATTERNS:
            # (A, B): the level forms x2 - x1 = B - A and sees `pat`; (B, A) sees the opposite pattern
            out.append((f"low_limb/{aname}/{pat}/fwd", A, found[pat]))
            out.append((f"low_limb/{aname}/{pat}/rev", found[pat], A))
    return out


SAME_Y_TRIPLES = 2


@functools.lru_cache(maxsize=None)
def same_y_triples(curve, group):
    """SAME_Y_TRIPLES triples of points on one horizontal line each: x^3 + a x + b - y^2 = (x - x1)(x^2 + x1 x + x1^2 + a)"""
    cv, deg = CURVES[curve], degree(curve, group)
    a = cv.coeff_a(group)
    half = pow(2, -1, cv.q)
    out = []
    for k in range(1, 1 + MAX_CANDIDATES):
        x1 = f_embed(cv, k, deg, 1)
        sq = cv.f_mul(x1, x1)
        disc = cv.f_neg(cv.f_add(f_scale(cv, sq, 3), f_scale(cv, a, 4)))
        s = f_sqrt(curve, disc)
        if s is None or cv.f_is_zero(s):
            continue
        p1 = lift(curve, group, x1)
        if p1 is None:
            continue
        x2 = f_scale(cv, cv.f_sub(s, x1), half)
        x3 = f_scale(cv, cv.f_neg(cv.f_add(s, x1)), half)
        if len({x1, x2, x3}) != 3:
            continue
        out.append(((x1, p1[1]), (x2, p1[1]), (x3, p1[1])))
        if len(out) == SAME_Y_TRIPLES:
            return tuple(out)
    raise LookupError(f"curve {curve}, G{group}: fewer than {SAME_Y_TRIPLES} same-y triples among {MAX_CANDIDATES} candidates")


def same_y(curve, group):
    out = []
    for t, tri in enumerate(same_y_triples(curve, group)):
        for i in range(3):
            for j in range(3):
                if i != j:
                    out.append((f"same_y/t{t}/P{i}+P{j}", tri[i], tri[j]))
                    out.append((f"same_y/t{t}/P{i}-P{j}", tri[i], neg(curve, tri[j])))
    return out


def _stored_pair(curve, base, d):
    """two points whose stored x residues are X and X + d, X the first of base + k 2^28 at which both lift and the stored integers
    differ by exactly d"""
    for k in range(MAX_CANDIDATES):
        X = base + (k << FR.LB)
        xa, xb = x_of_residue(curve, X), x_of_residue(curve, X + d)
        if stored(curve, xb) - stored(curve, xa) != d:
            continue
        pa = lift(curve, 1, xa)
        pb = lift(curve, 1, xb) if pa is not None else None
        if pb is not None:
            return pa, pb
    raise LookupError(f"curve {curve}: no liftable neighbours at distance {d}")


NEIGHBOUR_STORED = (("carry", MASK, (1, 2)), ("borrow", 0, (-1, -2)), ("plain", None, (1, 2)))
NEIGHBOUR_CANONICAL = (("small", 3), ("half", None))


@functools.lru_cache(maxsize=None)
def neighbour_x(curve):
    cv = CURVES[curve]
    XG = stored(curve, cv.gen(1)[0]) % cv.q
    out = []
    for kind, low, deltas in NEIGHBOUR_STORED:
        base = XG + (1 << FR.LB) if low is None else (XG & ~MASK) | low
        for d in deltas:
            pa, pb = _stored_pair(curve, base, d)
            out.append((f"neighbour_x/{kind}/{d:+d}/fwd", pa, pb))
            out.append((f"neighbour_x/{kind}/{d:+d}/rev", pb, pa))
    for kind, x0 in NEIGHBOUR_CANONICAL:
        x0 = (cv.q + 1) // 2 if x0 is None else x0
        for k in range(MAX_CANDIDATES):
            pa = lift(curve, 1, x0 + k)
            pb = lift(curve, 1, x0 + k + 1) if pa is not None else None
            if pb is not None:
                break
        else:
            raise LookupError(f"curve {curve}: no liftable canonical neighbours from {x0}")
        out.append((f"neighbour_x/canonical_{kind}/fwd", pa, pb))
        out.append((f"neighbour_x/canonical_{kind}/rev", pb, pa))
    return out


def edge_targets(curve):
    """[(name, "x" or "X", target, step)]: the walk from a target keeps what the target was chosen for (the low limb, limbs 0 .. 25)"""
    q = CURVES[curve].q
    return [("x=0", "x", 0, 1), ("x=1", "x", 1, 1), ("x=2", "x", 2, 1), ("x=q-2", "x", q - 2, -1), ("x=q-1", "x", q - 1, -1), ("x=(q-1)/2", "x", (q - 1) // 2, 1),
            ("X=0", "X", 0, 1), ("X=1", "X", 1, 1), ("X=2^28-1", "X", MASK, 1 << FR.LB), ("X=2^28", "X", 1 << FR.LB, 1 << FR.LB), ("X=one", "X", FR.RB % q, 1),
            ("X=q-1", "X", q - 1, -1), ("X=limbmax", "X", FR.val_std(FR.limb_max_below(q)), -(1 << (FR.LB * (FR.NL - 1))))]


EDGE_SMALL_LARGE = (("x=0", "x=q-1"), ("X=0", "X=q-1"), ("X=1", "X=limbmax"))


@functools.lru_cache(maxsize=None)
def edge_points(curve):
    """{target name: point}: the nearest liftable value at or after (step > 0) / at or before (step < 0) each target not taken already"""
    q = CURVES[curve].q
    taken, out = set(), collections.OrderedDict()
    for name, space, target, step in edge_targets(curve):
        walk = ((target + k * step) % q for k in itertools.count())
        xs = walk if space == "x" else (x_of_residue(curve, X) for X in walk)
        pt = first_liftable(curve, 1, (x for x in xs if x not in taken))
        taken.add(pt[0])
        out[name] = pt
    return out


def edge_x(curve):
    G = CURVES[curve].gen(1)
    pts = edge_points(curve)
    out = []
    for i, (name, pt) in enumerate(pts.items()):
        out.append((f"edge_x/{name}/gen", pt, G) if i % 2 == 0 else (f"edge_x/gen/{name}", G, pt))
    for lo, hi in EDGE_SMALL_LARGE:
        out.append((f"edge_x/{lo}/{hi}", pts[lo], pts[hi]))
        out.append((f"edge_x/{hi}/{lo}", pts[hi], pts[lo]))
    return out


# ---- G2 families --------------------------------------------------------------------------------------------------------------------------
def equal_components(x1, x2):
    return frozenset(i for i, (a, b) in enumerate(zip(x1, x2)) if a == b)


@functools.lru_cache(maxsize=None)
def partial_x(curve):
    cv = CURVES[curve]
    G = cv.gen(2)
    out = []
    for mask in range(1, (1 << cv.deg) - 1):
        keep = [i for i in range(cv.deg) if mask >> i & 1]
        cands = (tuple(g if i in keep else (g + k) % cv.q for i, g in enumerate(G[0])) for k in itertools.count(1))
        pt = first_liftable(curve, 2, cands)
        name = "".join(str(i) for i in keep)
        out.append((f"partial_x/eq{name}/fwd", G, pt))
        out.append((f"partial_x/eq{name}/rev", pt, G))
    return out


def sparse_masks(curve):
    """the sets of NON-zero components of x: one zero component, two (Fq3), the base field.  On the twist of MNT4753 (a' = (a nr, 0),
    b' = (0, b nr)) x = (0, t) gives x^3 + a' x + b' = (0, w), and (c + d i)^2 = (0, w) needs c^2 = -nr d^2: -1 is a square (q = 1 mod 4),
    nr is not, so no such x lifts -- Fq2 gets three base-field values, which are its x with one zero component"""
    return [(0,), (0,), (0,)] if CURVES[curve].deg == 2 else [(0, 1), (0, 2), (1, 2), (0,), (1,), (2,)]


@functools.lru_cache(maxsize=None)
def sparse_points(curve):
    cv = CURVES[curve]
    taken, out = set(), []
    for nz in sparse_masks(curve):
        cands = (tuple((3 + 2 * i + k) if i in nz else 0 for i in range(cv.deg)) for k in itertools.count())
        pt = first_liftable(curve, 2, (x for x in cands if x not in taken))
        taken.add(pt[0])
        out.append(("".join(str(i) for i in nz), pt))
    return out


def sparse_x(curve):
    G = CURVES[curve].gen(2)
    pts = sparse_points(curve)
    out = []
    for i, (nz, pt) in enumerate(pts):
        out.append((f"sparse_x/{i}nz{nz}/gen", pt, G) if i % 2 == 0 else (f"sparse_x/gen/{i}nz{nz}", G, pt))
    for i, (nz, pt) in enumerate(pts):                       # with each other: every unordered pair, the order alternating
        for j in range(i + 1, len(pts)):
            a, b = (i, j) if (i + j) % 2 else (j, i)
            out.append((f"sparse_x/{a}nz{pts[a][0]}/{b}nz{pts[b][0]}", pts[a][1], pts[b][1]))
    return out


def opposite(curve, group):
    cv = CURVES[curve]
    if group == 1:
        e = edge_points(curve)
        pts = [("gen", cv.gen(1)), ("lift", g1_anchors(curve)[1][1]), ("x=0", e["x=0"]), ("X=limbmax", e["X=limbmax"]), ("same_y", same_y_triples(curve, 1)[0][0])]
    else:
        sp = sparse_points(curve)
        pts = [("gen", cv.gen(2)), ("sparse_first", sp[0][1]), ("sparse_last", sp[-1][1]), ("same_y", same_y_triples(curve, 2)[0][0]), ("partial", partial_x(curve)[0][2])]
    return [(f"opposite/{n}/+-", pt, neg(curve, pt)) if i % 2 == 0 else (f"opposite/{n}/-+", neg(curve, pt), pt) for i, (n, pt) in enumerate(pts)]


# ---- the families of a group ----------------------------------------------------------------------------------------------------------------
# members per family, written down: low_limb 2 anchors x 3 patterns x 2 orders; same_y 2 triples x 6 ordered pairs x {+, -}; neighbour_x
# (2 + 2 + 2 stored + 2 canonical) x 2 orders; edge_x 13 targets with the generator + 3 small / large x 2 orders; partial_x (2^deg - 2)
# subsets x 2 orders; sparse_x one pair with the generator per point and every unordered pair of points (3 of 3 points in Fq2, 15 of 6 in Fq3);
# opposite 5 points
COUNTS = {(0, 1): dict(low_limb=12, same_y=24, neighbour_x=16, edge_x=19, opposite=5), (1, 1): dict(low_limb=12, same_y=24, neighbour_x=16, edge_x=19, opposite=5),
          (0, 2): dict(partial_x=4, same_y=24, sparse_x=6, opposite=5), (1, 2): dict(partial_x=12, same_y=24, sparse_x=21, opposite=5)}
TOTALS = {(0, 1): 76, (1, 1): 76, (0, 2): 39, (1, 2): 62}


@functools.lru_cache(maxsize=None)
def families_points(curve, group):
    """{family: [(name, P, Q)]} with P, Q as pyref points"""
    if group == 1:
        fams = [("low_limb", low_limb(curve)), ("same_y", same_y(curve, 1)), ("neighbour_x", neighbour_x(curve)), ("edge_x", edge_x(curve)), ("opposite", opposite(curve, 1))]
    else:
        fams = [("partial_x", partial_x(curve)), ("same_y", same_y(curve, 2)), ("sparse_x", sparse_x(curve)), ("opposite", opposite(curve, 2))]
    return collections.OrderedDict(fams)


@functools.lru_cache(maxsize=None)
def families(curve, group):
    """{family: [Member(name, P, Q)]} in affine wire words (read-only arrays)"""
    out = collections.OrderedDict()
    for fam, mem in families_points(curve, group).items():
        rows = []
        for name, P, Q in mem:
            p, q = to_words(curve, group, P), to_words(curve, group, Q)
            p.setflags(write=False); q.setflags(write=False)
            rows.append(Member(name, p, q))
        out[fam] = rows
    return out


def members(curve, group, only=None):
    return [m for fam, mem in families(curve, group).items() if only is None or fam in only for m in mem]


def members_points(curve, group, only=None):
    return [m for fam, mem in families_points(curve, group).items() if only is None or fam in only for m in mem]


def distinct_points(curve, group):
    """every designed point of the group once, in order of first appearance"""
    seen, out = set(), []
    for _, P, Q in members_points(curve, group):
        for pt in (P, Q):
            if pt not in seen:
                seen.add(pt)
                out.append(pt)
    return out


# ---- projective representatives ---------------------------------------------------------------------------------------------------------------
LAMBDAS = ("q-1", "uniform", "1/X")      # besides Z = 1


def lambdas(curve, group, family, pt, seed):
    """{name: lam}: -1, a uniform element and the inverse of X (a coordinate becomes 1).  For partial_x lam stays in the base field, so
    that the partial zero of x2 - x1 survives the scaling (there 1 / x_0: component 0 of X becomes 1)."""
    cv = CURVES[curve]
    deg = degree(curve, group)
    rng = pyref.splitmix64(seed)
    base_only = family == "partial_x"
    uni = pyref.rand_below(rng, cv.q - 1) + 1
    if deg > 1:
        uni = tuple([uni] + [0 if base_only else pyref.rand_below(rng, cv.q) for _ in range(deg - 1)])
    x = pt[0]
    if base_only:
        inv = f_embed(cv, pow(x[0], -1, cv.q), deg)
    else:
        inv = cv.f_inv(x if not cv.f_is_zero(x) else pt[1])        # x = 0: Y becomes 1 instead
    return {"q-1": f_embed(cv, cv.q - 1, deg), "uniform": uni, "1/X": inv}


# ---- MSM inputs: every pair in a bucket of its own (the affine pair addition of the levels, the accumulate walk) ------------------------------
def pair_bucket_input(curve, group, c, table):
    """(bases [n, words], scalars as integers, {key: (member index, flagged copy?)}): member i's bases both get the scalar j, a bucket
    number of their own; a second copy gives the second base 2^c - j instead -- digit -j and a carry --, so the sign-flag paths see
    (P, -Q).  j starts at 2: bucket 1 (of the next window) takes the carries.  With the window table every j is a digit of window 0; without
    it (key = w nb + |d| - 1) the pairs spread over the even windows and the carries land in bucket 1 of the odd ones."""
    mem = members(curve, group)
    nb = 1 << (c - 1)
    per_window = nb - 2
    bases, ints, keys = [], [], {}
    for copy in (0, 1):
        for i, m in enumerate(mem):
            slot = copy * len(mem) + i
            w, j = (0, slot + 2) if table else (2 * (slot // per_window), 2 + slot % per_window)
            assert 2 <= j < nb and w + 1 < S.windows(c) - 1
            bases += [m.P, m.Q]
            ints += [j << (w * c), ((1 << c) - j if copy else j) << (w * c)]
            keys[(0 if table else w * nb) + j - 1] = (i, bool(copy))
    return np.stack(bases), ints, keys


def _knobs(pairs, irrs, tmins):
    return M.run_order(M.knob_product(pairs, irrs, tmins, sort="part") + M.knob_product(pairs, irrs, tmins, sort="atomic"))


# PAIR 0: the straight-line mixed addition of k_bucket_accumulate adds the pair; PAIR 1 .. 3: the first level does.  (Without the table,
# at c = 7, the partition passes do not apply -- msm_occupancy.partition_fits -- and a `part` setting takes the atomic sort: the list is
# kept as it is for both modes, and there the `part` half repeats the `atomic` half's work and adds no coverage; the sort stage is not in
# the reported plan, so the plan check cannot tell the two apart.)
PAIR_BUCKET_KNOBS = {1: _knobs((0, 1, 2, 3), (0, 1), (1, 8)), 2: _knobs((0, 2), (0, 1), (1, 8))}


def pair_bucket_cases(curve, group):
    """[msm_occupancy.Case]: G1 in table mode (c = 12) and without the table (c = 7), G2 in table mode; build(curve) -> pair_bucket_input"""
    out = [M.Case("pairs_table", lambda curve: pair_bucket_input(curve, group, M.C_TABLE, True), PAIR_BUCKET_KNOBS[group], M.C_TABLE, True)]
    if group == 1:
        out.append(M.Case("pairs_no_table", lambda curve: pair_bucket_input(curve, group, M.C_NO_TABLE, False), PAIR_BUCKET_KNOBS[group], M.C_NO_TABLE, False))
    return out


# ---- MSM inputs: P and Q alone in two buckets whose keys differ in one bit (the full additions of the reduction) -----------------------------
REDUCTION_FAMILIES = ("same_y", "partial_x", "edge_x", "opposite")


def reduction_keys(i, bit, c):
    """keys (bucket number - 1) of P and Q of member i: they differ in `bit` alone.  The first key is below 2^(c-3): two zero bits at the
    top, so that neither key is 2^(c-1) - 1, the extreme digit with its carry"""
    kb = (5 * i + 3) % (1 << (c - 3))
    return kb, kb ^ (1 << bit)


def reduction_scalars(n_members, i, bit, c):
    """the scalars of the base set [P_0, Q_0, P_1, Q_1, ...]: zero but for member i's two"""
    ints = [0] * (2 * n_members)
    kp, kq = reduction_keys(i, bit, c)
    ints[2 * i], ints[2 * i + 1] = kp + 1, kq + 1
    return ints


# ---- MSM inputs: one bucket of 2T + 1 entries that holds P, Q and copies of a third point (the edge merge) ------------------------------------
EDGE_BUCKET = 9           # the bucket number
EDGE_TMINS = (1, 4)


def third_point(curve, group):
    cv = CURVES[curve]
    return cv.mul(3, cv.gen(group), group)


def edge_merge_scalars(n_members, i, T):
    """the scalars of the base set [P_0, Q_0, P_1, Q_1, ..., R x (2 max(EDGE_TMINS) - 1)]: member i's two points and 2T - 1 copies of
    the third point share the bucket EDGE_BUCKET, 2T + 1 entries in all"""
    ints = [0] * (2 * n_members + 2 * max(EDGE_TMINS) - 1)
    ints[2 * i] = ints[2 * i + 1] = EDGE_BUCKET
    for k in range(2 * T - 1):
        ints[2 * n_members + k] = EDGE_BUCKET
    return ints
