"""Expected values and scalar families of the fixed-base batch scalar multiplication tests (TEST INFRASTRUCTURE).

Sources of expected values, in order of authority: (a) libff-minted goldens (golden_io.group / golden_io.msm with n = 1), (b) the CPU
oracle's scalar multiplication, one call per value and cached, (c) the MSM fold for everything bulk: the outputs Q_k = e_k P become a
base set, an MSM with uniform s_k over it must equal (sum s_k e_k mod r) P from ONE oracle call.  The MSM is pinned to libff by its
own tests and shares no kernel with the walk; one wrong output changes the sum."""
import numpy as np

import domain_ref as D
import msm_structured as S
import oracle_lib as O

_ORACLE = {}


def modulus(curve):
    return D.MODULUS[curve]


def wire(curve, ints):
    """uint64 [n, 12], Montgomery form; an empty list gives shape (0, 12)"""
    if len(ints) == 0:
        return np.zeros((0, 12), dtype=np.uint64)
    return np.ascontiguousarray(D.to_wire(curve, list(ints)), dtype=np.uint64).reshape(-1, 12)


def wrap_family(curve):
    """[(k, s_k)] for k = 700 .. 752 with r mod 2^k < 2^(k-1):  s_k = 2 floor(r / 2^k) 2^k - r = floor(r / 2^k) 2^k - (r mod 2^k).
    With signed digits the partial sum below bit k is -(r mod 2^k) and the digits above it name floor(r / 2^k) 2^k P -- the same point,
    the two differ by r: a walk meets an accumulator equal (or, from the other end, related by r) to its row, and only a complete
    addition survives."""
    r, out = modulus(curve), []
    for k in range(700, 753):
        q, m = r >> k, r & ((1 << k) - 1)
        if m < (1 << (k - 1)):
            out.append((k, (q << k) - m))
    return out


def oracle_scale(curve, group, point, s):
    """(b): s * point by the oracle, affine wire words; cached per (curve, group, point, s)"""
    point = np.ascontiguousarray(point, dtype=np.uint64)
    key = (curve, group, point.tobytes(), int(s))
    if key not in _ORACLE:
        v = O.point_op(curve, group, 3, point, wire(curve, [s])[0])
        v.setflags(write=False)
        _ORACLE[key] = v
    return _ORACLE[key]


def neg_point(curve, group, aff):
    """-(x, y) in affine wire words (the identity, all zero, stays)"""
    aff = np.array(aff, dtype=np.uint64)
    half = aff.size // 2
    if not aff[half:].any():
        return aff
    aff[half:] = O.neg_fq(curve, aff[half:]) if group == 1 else O.ext_op(curve, 5, aff[half:])
    return aff


def fold_check(pkg, curve, group, point, ints, outs, seed, what):
    """(c): MSM of the outputs with uniform scalars against one oracle call; on a mismatch names the first wrong output"""
    n = len(ints)
    assert outs.shape == (n, O.aff_words(curve, group)), (what, outs.shape)
    if n == 0:
        return
    sk = pkg.synth_scalars(curve, seed, n)
    sk_int = D.from_wire(curve, sk)
    bs = pkg.BaseSet(curve, group, outs)
    try:
        got = pkg.point_to_affine(curve, group, bs.msm(sk))
    finally:
        bs.close()
    total = sum(int(a) * int(e) for a, e in zip(sk_int, ints)) % modulus(curve)
    if np.array_equal(got, oracle_scale(curve, group, point, total)):
        return
    proj = pkg.point_from_affine(curve, group, point)
    for k, e in enumerate(ints):
        exp = pkg.point_to_affine(curve, group, pkg.point_scale(curve, group, wire(curve, [e])[0], proj))
        if not np.array_equal(exp, outs[k]):
            raise AssertionError(f"{what}: output {k} of {n} (scalar {hex(e)}) is not scalar * P")
    raise AssertionError(f"{what}: the fold differs although every output equals point_scale")


def structured(curve, c, with_single_bits=False):
    """[(label, integers)]: the families of tests/msm_structured.py at width c"""
    names = ["extremes", "carry_chains", "edges", "dense"] + (["single_bits"] if with_single_bits else [])
    return [(S.label(name, c), S.family(curve, name, c)) for name in names]


def anchors(curve, widths):
    """the scalars every width is checked on by the oracle directly: the ends of the field, 2^752, and the extremes of the top window of
    every width in `widths`"""
    r = modulus(curve)
    out = [0, 1, 2, r - 1, r - 2, 1 << 752]
    for c in widths:
        for v in S.extremes(curve, c)[-2:]:
            if v not in out:
                out.append(v)
    return out
