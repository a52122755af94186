"""Subgroup membership on the twists of MNT4753 / MNT6753 in Python integers.

G2 is the order-r subgroup of E'(F), F = Fq2 / Fq3; both twists have a large cofactor.  With psi = twist^-1 o Frobenius_q o twist,
    psi(x, y) = (x^q gamma_1^-2, y^q gamma_1^-3),   gamma_1 = NR^((q - 1) / k),
psi satisfies X^2 - t X + q (t = q + 1 - r, G1 has cofactor 1) and G2 is its eigenspace of the eigenvalue q = t - 1 (mod r), so
    P in G2  <=>  psi(P) == [t - 1] P,   t - 1 = q - r: the signed ate loop count.
Nothing here is the project's arithmetic: F elements are tuples of residues (tools/pyref.py), the multiple is pyref's affine
double-and-add, which is complete.  tests/test_subgroup_cpu.py checks the test against the definition [r] P == O.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pyref  # noqa: E402
import designed_points as DP  # noqa: E402

CURVES = {0: pyref.Curve(0), 1: pyref.Curve(1)}
GROUPS_PER_WAVE = {0: 32, 1: 21}      # lane groups of one wave: 2 lanes per point on MNT4753, 3 on MNT6753 (lane 63 idle)


def gamma1(curve):
    C = CURVES[curve]
    return pow(C.nr, (C.q - 1) // (2 * C.deg), C.q)


def loop_multiplier(curve):
    """t - 1 = q - r, signed"""
    C = CURVES[curve]
    return C.q - C.r


def frobenius_f(curve, x):
    """x^q in F = Fq[u] / (u^deg - NR): u^q = NR^((q - 1) / deg) u = gamma_1^2 u"""
    C, g = CURVES[curve], gamma1(curve)
    return tuple(v * pow(g, 2 * c, C.q) % C.q for c, v in enumerate(x))


def psi(curve, pt):
    if pt is None:
        return None
    C, g = CURVES[curve], gamma1(curve)
    kx, ky = pow(g, -2, C.q), pow(g, -3, C.q)
    return (tuple(v * kx % C.q for v in frobenius_f(curve, pt[0])), tuple(v * ky % C.q for v in frobenius_f(curve, pt[1])))


def signed_mul(curve, k, pt):
    C = CURVES[curve]
    res = C.mul(abs(k), pt, 2)
    return C.neg(res) if k < 0 else res


def loop_multiple(curve, pt):
    """[t - 1] P"""
    return signed_mul(curve, loop_multiplier(curve), pt)


def in_subgroup(curve, pt):
    """the test the device runs; the identity is a member"""
    return pt is None or psi(curve, pt) == loop_multiple(curve, pt)


def in_subgroup_by_definition(curve, pt):
    return CURVES[curve].mul(CURVES[curve].r, pt, 2) is None


# ---- points -------------------------------------------------------------------------------------------------------------------------
def lifted(curve, count, start=2):
    """`count` points of the twist E'(F) lifted from small x = (c, 1[, 0]) (designed_points.lift): deterministic; with a cofactor
    of some 750 (MNT4753) / 1500 (MNT6753) bits none of them is in G2, which the CPU test asserts."""
    C, out, c = CURVES[curve], [], start
    while len(out) < count:
        x = (c, 1) if C.deg == 2 else (c, 1, 0)
        pt = DP.lift(curve, 2, x)
        if pt is not None:
            out.append(pt)
        c += 1
    return out


def generator_multiple(curve, k):
    C = CURVES[curve]
    return C.mul(k, C.gen(2), 2)


def cofactor_part(curve, pt):
    """[r] P: in the cofactor group, of order prime to r"""
    return CURVES[curve].mul(CURVES[curve].r, pt, 2)


_CACHE = {}


def off_subgroup_points(curve):
    """A fixed list of twist points outside G2, computed once per process: three lifted points P, their cofactor parts T = [r] P, and
    Q + T for Q in G2."""
    if curve not in _CACHE:
        C = CURVES[curve]
        ps = lifted(curve, 3)
        ts = [cofactor_part(curve, p) for p in ps]
        qs = [C.add(generator_multiple(curve, 5 + i), t, 2) for i, t in enumerate(ts)]
        _CACHE[curve] = {"lifted": ps, "cofactor": ts, "mixed": qs}
    return _CACHE[curve]


def words(curve, pt):
    return np.array(CURVES[curve].affine_to_words(pt, 2), dtype=np.uint64)


def from_words(curve, w):
    return CURVES[curve].affine_from_words([int(v) for v in w], 2)
