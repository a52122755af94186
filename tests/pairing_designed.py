"""DESIGNED inputs for the pairing stack (TEST INFRASTRUCTURE, pure Python over tools/pyref.py, pairing_ref.py, designed_points.py and
subgroup_ref.py): tower elements and Miller pairs with planted structure, with the model's answers.

Everything else the suite feeds to the tower (csrc/tower753.hip.h), to Ate<C> and to the kernels of csrc/pairing_kernels.hip.h is
uniform for practical purposes.  The families here plant what a uniform value never shows.  A member has a name; every lookup goes
through `member` / `miller_pair`, which raise KeyError; COUNTS fixes the size of every family and `families` asserts it, so no member is
ever dropped quietly.  tests/test_pairing_designed_cpu.py checks every claim made here and runs the families through the one-lane host
build; tests/test_pairing_designed_gpu.py runs them on the device in both forms.

Tower elements, per curve (F = Fq2 / Fq3, deg = 2 / 3; an element is (c0, c1) over F, 2 deg components over Fq):
    edge      one value in ALL components: canonical 0, 1, 2, q-2, q-1, (q-1)/2, (q+1)/2 and the values whose stored residue X' = x R'
              (what fp_from_wire leaves in the limbs, designed_points.edge_targets) is 1, 2^28 - 1, 2^28, R' mod q, q - 1 and the largest
              value below q with limbs 0 .. 25 all 0xFFFFFFF ("X=one" is the canonical value 1 again: kept under its own name, the table
              counts it); and q-1 and (q-1)/2 in ONE component, uniform values in the rest, at every component position
    subfield  c1 = 0 (an element of F), only c0.c0 non-zero (an element of Fq), c0 = 0 (v F), and -1
    unitary   conj(y) / y for uniform y (norm one over F), first-chunk values (the cyclotomic subgroup), and e(G1, G2)^j for
              j = 1, 2, r - 1 (order r)
    pairs     operand pairs for mul: (a, 1/a) -> the element 1, (a, conj a) -> the norm, c1 exactly the zero words, (a, -a), (a, 1), (a, 0)

Miller pairs, per curve, at most MAX_PAIRS = 48, the model's unreduced value and pairing computed once per process:
    every G1 point of designed_points.edge_points with G2::one() and with one designed_points.sparse_points member (taken in turn);
    G1::one() with G2::one(), with every sparse_points member (zero components in x, x in the base field: off the subgroup), with every
    point of subgroup_ref.off_subgroup_points (lifted, cofactor, mixed), with -G2::one() and [2] G2::one();
    the sign table: (-P, Q) and (P, -Q) of the generator pair, of (G1::one(), -G2::one()) and of the pair of the edge point x=0 with
    G2::one() -- the generators in all four sign combinations.

Out of scope, on purpose: twist points whose stepping meets Z = 0 in mid-loop (a component of small order in the cofactor group).
tests/test_subgroup_gpu.py covers the stepping there, and the Miller value has no meaning in that case; `stepping_never_meets_zero`
shows that no point used here is one of them.  The final exponentiation of zero is unspecified and is no member's expected value.
"""
import collections
import functools
import os

import numpy as np

import designed_points as DP
import pairing_ref as PR
import pyref
import subgroup_ref as SG

Elem = collections.namedtuple("Elem", "name value")            # value: ((c0 components), (c1 components)) as integers
OpPair = collections.namedtuple("OpPair", "name a b")
MillerPair = collections.namedtuple("MillerPair", "name P Q")  # pyref affine points

MAX_PAIRS = 48
UNIFORM_SEED = 7530
SINGLE_VALUES = ("q-1", "(q-1)/2")
PAIR_KINDS = ("inverse", "conjugate", "negative", "one", "zero")
ORDER_R_POWERS = ("1", "2", "r-1")

# members per family, written down: edge 7 canonical + 6 stored-residue values in all components and 2 values x 2 deg positions;
# subfield 4; unitary 2 conj(y) / y + 2 first-chunk values + 3 powers of e(G1, G2); pairs 3 elements a x 5 kinds
COUNTS = {0: dict(edge=13 + 2 * 4, subfield=4, unitary=7, pairs=15), 1: dict(edge=13 + 2 * 6, subfield=4, unitary=7, pairs=15)}
# Miller pairs: 13 edge points x 2, the generator pair, the sparse points (3 / 6), 9 off the subgroup, -G2::one() and [2] G2::one(), and
# the 4 negated pairs that are not members already
MILLER_COUNTS = {0: 26 + 1 + 3 + 9 + 2 + 4, 1: 26 + 1 + 6 + 9 + 2 + 4}
SIGN_BASES = ("gen/gen", "gen/-gen", "edge/x=0/gen")


@functools.lru_cache(maxsize=None)
def model(curve):
    return PR.Pairing(curve)


def canonical_values(curve):
    q = model(curve).q
    return [("0", 0), ("1", 1), ("2", 2), ("q-2", q - 2), ("q-1", q - 1), ("(q-1)/2", (q - 1) // 2), ("(q+1)/2", (q + 1) // 2)]


def stored_values(curve):
    """[(name, x)]: the canonical x whose stored residue x R' mod q is the target X of designed_points.edge_targets (X = 0 is x = 0)"""
    out = [(name, DP.x_of_residue(curve, target)) for name, space, target, _ in DP.edge_targets(curve) if space == "X" and name != "X=0"]
    assert [n for n, _ in out] == ["X=1", "X=2^28-1", "X=2^28", "X=one", "X=q-1", "X=limbmax"]
    return out


def shape(curve, flat):
    """2 deg components, c0 first -> a tower element"""
    d = model(curve).deg
    assert len(flat) == 2 * d
    return (tuple(flat[:d]), tuple(flat[d:]))


def flat(elem):
    return list(elem[0]) + list(elem[1])


def uniform(curve, k):
    """the k-th uniform tower element of the curve (deterministic)"""
    P = model(curve)
    rng = pyref.splitmix64(UNIFORM_SEED + 100 * curve + k)
    return shape(curve, [pyref.rand_below(rng, P.q) for _ in range(2 * P.deg)])


@functools.lru_cache(maxsize=None)
def generator_pairing(curve):
    P = model(curve)
    return P.reduced_pairing(P.C.gen(1), P.C.gen(2))


def _edge(curve):
    P = model(curve)
    out = [Elem(f"edge/all/{n}", shape(curve, [v] * (2 * P.deg))) for n, v in canonical_values(curve) + stored_values(curve)]
    vals = dict(canonical_values(curve))
    for n in SINGLE_VALUES:
        for pos in range(2 * P.deg):
            comps = flat(uniform(curve, 10 + pos))
            comps[pos] = vals[n]
            out.append(Elem(f"edge/one/{n}/c{pos // P.deg}.c{pos % P.deg}", shape(curve, comps)))
    return out


def _subfield(curve):
    P = model(curve)
    u = uniform(curve, 30)
    return [Elem("subfield/F", (u[0], P.f_zero)), Elem("subfield/Fq", (P.f_embed(u[0][0]), P.f_zero)), Elem("subfield/vF", (P.f_zero, u[1])),
            Elem("subfield/-1", (P.C.f_neg(P.f_one), P.f_zero))]


def _unitary(curve):
    P = model(curve)
    out = []
    for k in range(2):
        y = uniform(curve, 40 + k)
        out.append(Elem(f"unitary/conj_over/{k}", P.mul(P.conj(y), P.inv(y))))
    for k in range(2):
        y = uniform(curve, 50 + k)
        out.append(Elem(f"unitary/first_chunk/{k}", P.first_chunk(y, P.inv(y))))
    e = generator_pairing(curve)
    powers = {"1": 1, "2": 2, "r-1": P.C.r - 1}
    out += [Elem(f"unitary/order_r/{n}", P.pow(e, powers[n])) for n in ORDER_R_POWERS]
    return out


def _pairs(curve):
    P = model(curve)
    zero = (P.f_zero, P.f_zero)
    bases = [("uniform0", uniform(curve, 60)), ("uniform1", uniform(curve, 61)), ("unitary", _unitary(curve)[0].value)]
    out = []
    for n, a in bases:
        partner = {"inverse": P.inv(a), "conjugate": P.conj(a), "negative": (P.C.f_neg(a[0]), P.C.f_neg(a[1])), "one": P.one(), "zero": zero}
        out += [OpPair(f"pairs/{n}/{kind}", a, partner[kind]) for kind in PAIR_KINDS]
    return out


@functools.lru_cache(maxsize=None)
def families(curve):
    """{family: [Elem]} (and [OpPair] for `pairs`), sizes as COUNTS, names unique"""
    out = collections.OrderedDict([("edge", _edge(curve)), ("subfield", _subfield(curve)), ("unitary", _unitary(curve)), ("pairs", _pairs(curve))])
    assert {k: len(v) for k, v in out.items()} == COUNTS[curve], {k: len(v) for k, v in out.items()}
    names = [m.name for v in out.values() for m in v]
    assert len(set(names)) == len(names)
    return out


def elements(curve, only=("edge", "subfield", "unitary")):
    """[Elem] of the element families named, in order"""
    fam = families(curve)
    return [m for name in only for m in fam[name]]       # KeyError on a family that does not exist


def member(curve, name):
    for fam in families(curve).values():
        for m in fam:
            if m.name == name:
                return m
    raise KeyError(f"curve {curve}: no designed tower member {name!r}")


def is_zero(curve, value):
    P = model(curve)
    return value == (P.f_zero, P.f_zero)


def words(curve, values):
    """tower elements (integers) -> [n, gt_words] wire words"""
    P = model(curve)
    return np.stack([P.gt_to_words(v) for v in values])


def norm(curve, a):
    """a conj(a) = c0^2 - u c1^2, an element of F"""
    P = model(curve)
    return P.C.f_sub(P.f_sqr(a[0]), P.f_mul_by_u(P.f_sqr(a[1])))


def expected(curve, op, a, b=None):
    """the model's answer to operation `op` of mnt753_test_tower_op (0 -> 0 for the inverse)"""
    P = model(curve)
    if op == 0:
        return P.mul(a, b)
    if op == 1:
        return P.sqr(a)
    if op == 2:
        return a if is_zero(curve, a) else P.inv(a)
    if op == 3:
        return P.conj(a)
    if op == 4:
        return P.pow(a, P.K["w0_abs"])
    if op == 5:
        if is_zero(curve, a):
            raise ValueError("the final exponentiation of zero is unspecified")
        return P.final_exponentiation(a)
    if 11 <= op < 10 + P.k:
        return P.frobenius(a, op - 10)
    raise KeyError(f"no tower operation {op}")


# ---- Miller pairs -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def miller_pairs(curve):
    """[MillerPair], MILLER_COUNTS[curve] <= MAX_PAIRS of them, names unique"""
    C = model(curve).C
    g1, g2 = C.gen(1), C.gen(2)
    sparse = DP.sparse_points(curve)
    out = []
    for i, (name, pt) in enumerate(DP.edge_points(curve).items()):
        out.append(MillerPair(f"edge/{name}/gen", pt, g2))
        nz, sp = sparse[i % len(sparse)]
        out.append(MillerPair(f"edge/{name}/sparse{i % len(sparse)}nz{nz}", pt, sp))
    out.append(MillerPair("gen/gen", g1, g2))
    out += [MillerPair(f"gen/sparse{i}nz{nz}", g1, sp) for i, (nz, sp) in enumerate(sparse)]
    off = SG.off_subgroup_points(curve)
    for kind in ("lifted", "cofactor", "mixed"):
        out += [MillerPair(f"gen/{kind}{i}", g1, pt) for i, pt in enumerate(off[kind])]
    out.append(MillerPair("gen/-gen", g1, C.neg(g2)))
    out.append(MillerPair("gen/2gen", g1, C.add(g2, g2, 2)))
    byname = {m.name: m for m in out}
    have = {(m.P, m.Q) for m in out}
    for base in SIGN_BASES:
        b = byname[base]
        for tag, pr in (("-P", (C.neg(b.P), b.Q)), ("-Q", (b.P, C.neg(b.Q)))):
            if pr not in have:                   # (gen, -gen) and (gen, gen) are each other's (P, -Q)
                have.add(pr)
                out.append(MillerPair(f"neg/{base}/{tag}", *pr))
    assert len(out) == MILLER_COUNTS[curve] <= MAX_PAIRS, len(out)
    assert len({m.name for m in out}) == len(out)
    return out


def miller_pair(curve, name):
    for m in miller_pairs(curve):
        if m.name == name:
            return m
    raise KeyError(f"curve {curve}: no designed Miller pair {name!r}")


def miller_index(curve, P, Q):
    """the position of the pair (P, Q) among miller_pairs; KeyError where it is no member"""
    for i, m in enumerate(miller_pairs(curve)):
        if (m.P, m.Q) == (P, Q):
            return i
    raise KeyError(f"curve {curve}: the pair is not a designed Miller pair")


def sign_table(curve):
    """[(base, index of (P, Q), of (-P, Q), of (P, -Q))] for SIGN_BASES"""
    C = model(curve).C
    out = []
    for base in SIGN_BASES:
        b = miller_pair(curve, base)
        out.append((base, miller_index(curve, b.P, b.Q), miller_index(curve, C.neg(b.P), b.Q), miller_index(curve, b.P, C.neg(b.Q))))
    return out


# ML(-P, Q) = ML(P, -Q) = sign * conj(ML(P, Q)): +conj on MNT6753, -conj on MNT4753 (negative loop count: a closing step and an
# inversion).  tests/test_pairing_designed_cpu.py pins the signs in the model; the GPU tests use them between the device's own outputs.
RELATION_SIGN = {0: -1, 1: +1}


def signed_conj(curve, f, sign):
    P = model(curve)
    c = P.conj(f)
    return c if sign > 0 else (P.C.f_neg(c[0]), P.C.f_neg(c[1]))


def miller_words(curve):
    """(G1 points [n, 24], G2 points [n, affine words]) of miller_pairs, wire words"""
    C = model(curve).C
    prs = miller_pairs(curve)
    return (np.array([C.affine_to_words(m.P, 1) for m in prs], dtype=np.uint64), np.array([C.affine_to_words(m.Q, 2) for m in prs], dtype=np.uint64))


@functools.lru_cache(maxsize=None)
def miller_values(curve):
    """the model's unreduced Miller value of every pair, as tower elements: computed once per process, shared by both forms"""
    P = model(curve)
    return tuple(P.miller(m.P, m.Q) for m in miller_pairs(curve))


@functools.lru_cache(maxsize=None)
def pairing_values(curve):
    """the model's reduced pairing of every pair"""
    P = model(curve)
    return tuple(P.final_exponentiation(f) for f in miller_values(curve))


def stepping_never_meets_zero(curve, Q):
    """the running point of the Miller loop on Q keeps Z != 0 at every step (the closing step of a negative loop count, which ends at
    the identity by construction, left out)"""
    P = model(curve)
    qy2 = P.f_sqr(Q[1])
    R = (Q[0], Q[1], P.f_one, P.f_one)
    for bit in P.loop_bits():
        R, _ = P.dbl_step(R)
        if P.C.f_is_zero(R[2]):
            return False
        if bit == "1":
            R, _ = P.add_step(Q[0], Q[1], qy2, R)
            if P.C.f_is_zero(R[2]):
                return False
    return True


# ---- the Groth16 fixture of the near-miss tests ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def g16_fixture(curve):
    """(alpha_g1, beta_g2, delta_g2, ABC[0] | ABC[1], the valid proof, its public input) of tests/golden/g16_mnt{4,6}, wire words:
    keys.bin, the '0'-prefixed points of vk.txt (pairing_ref.serialize_vk's layout with one input), full.bin and input.bin"""
    name = f"g16_mnt{4 if curve == 0 else 6}"
    path = lambda f: os.path.join(PR.GOLDEN, name, f)
    w2 = 24 * model(curve).deg
    alpha, beta = PR.alpha_beta_words(name)
    delta = PR.delta_words(name)
    raw = open(path("vk.txt"), "rb").read()
    at = 8 * w2 + 1 + 8 * w2                     # GT | '0' delta
    head = b"1\n1\n0\n1\n"
    assert raw[at:at + 1] == b"0" and raw[at + 193:at + 193 + len(head) + 1] == head + b"0" and len(raw) == at + 193 + len(head) + 193
    words = lambda b: np.frombuffer(b, dtype="<u8").astype(np.uint64)
    abc = np.concatenate([words(raw[at + 1:at + 193]), words(raw[at + 194 + len(head):])])
    assert PR.serialize_vk(curve, PR.vk_head(name), delta, abc) == raw
    proof = np.fromfile(path("full.bin"), dtype="<u8").astype(np.uint64)
    inp = np.fromfile(path("input.bin"), dtype="<u8", count=24).astype(np.uint64)[12:]
    return alpha, beta, delta, abc, proof, inp


# ---- lane placement -----------------------------------------------------------------------------------------------------------------------
LAUNCH = {0: 129, 1: 86}              # a workgroup of lane groups (128 / 84) and a ragged tail
WAVE_GROUPS = {0: 32, 1: 21}          # lane groups of one wave (lane 63 idles on MNT6753)


def placement(curve, count, rotate):
    """indices into a family of `count` members for one launch of LAUNCH[curve] elements: the family cycled, `rotate` waves of groups on"""
    return (np.arange(LAUNCH[curve]) + rotate * WAVE_GROUPS[curve]) % count
