"""The spot check of compute_H in Python integers: H(t) Z(t) = A(t) B(t) - C(t) at one point t, on top of domain_ref.py, qap_ref.py
and mixed_domain_ref.py.

With m the size of the domain and u = L(t) its Lagrange coefficients at t (qap_ref.lagrange_fast),
    A(t) = sum ca_i u_i,  B(t) = sum cb_i u_i,  C(t) = sum cc_i u_i          (i < m)
    H(t) = sum h_i t^i over all m + 1 coefficients compute_h writes (the appended zero included)
    Z(t) = the vanishing polynomial of the domain (qap_ref.vanishing)
and the check is A(t) B(t) - C(t) == Z(t) H(t) in Fr.  Integers are plain residues in [0, r); domain_ref.from_wire / to_wire convert.
The device calls this models: mnt753_vec_dot, mnt753_poly_eval, mnt753_domain_interp_at, mnt753_h_check, mnt753_compute_h_checked.
"""
import random

import numpy as np

import domain_ref as D
import mixed_domain_ref as MX
import qap_ref as Q

BASIC, EXTENDED, STEP, MIXED = D.BASIC, D.EXTENDED, D.STEP, D.MIXED


def dot(a, b, r):
    return sum(x * y for x, y in zip(a, b)) % r


def poly_eval(c, t, r):
    acc = 0
    for v in reversed(c):
        acc = (acc * t + v) % r
    return acc


def interp_at(curve, kind, m, t, vecs):
    """the values at t of the polynomials of degree < m that take vecs[j][i] at the domain's i-th element"""
    r = D.MODULUS[curve]
    u = Q.lagrange_fast(curve, kind, m, t)
    return [dot(v, u, r) for v in vecs]


def sides(curve, kind, m, t, ca, cb, cc, h):
    """(A(t) B(t) - C(t), Z(t) H(t)); ca, cb, cc: m integers each, h: m + 1"""
    r = D.MODULUS[curve]
    assert len(ca) == len(cb) == len(cc) == m and len(h) == m + 1
    a, b, c = interp_at(curve, kind, m, t, (ca, cb, cc))
    return (a * b - c) % r, Q.vanishing(curve, kind, m, t) * poly_eval(h, t, r) % r


def holds(curve, kind, m, t, ca, cb, cc, h):
    lhs, rhs = sides(curve, kind, m, t, ca, cb, cc, h)
    return lhs == rhs


def compute_h_wire(curve, kind, m, ca_w, cb_w, cc_w):
    """compute_H on wire arrays [m, 12] -> [m + 1, 12], every kind of domain"""
    if kind == MIXED:
        assert curve == 1
        return MX.fast_compute_h(m, ca_w, cb_w, cc_w)
    return D.fast_compute_h_wire(curve, kind, m, ca_w, cb_w, cc_w)


def satisfied_rows(curve, m, seed):
    """m random rows with ca_i cb_i = cc_i, as integers"""
    r = D.MODULUS[curve]
    rng = random.Random(seed)
    ca = [rng.randrange(r) for _ in range(m)]
    cb = [rng.randrange(r) for _ in range(m)]
    return ca, cb, [x * y % r for x, y in zip(ca, cb)]


def random_t(curve, seed):
    return random.Random(seed).randrange(D.MODULUS[curve])


def wire1(curve, v):
    """one integer -> 12 uint64 in wire form"""
    return np.ascontiguousarray(D.to_wire(curve, [v])[0], dtype=np.uint64)


def unwire1(curve, words):
    return D.from_wire(curve, np.asarray(words, dtype=np.uint64).reshape(1, 12))[0]
