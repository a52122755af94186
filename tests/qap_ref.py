"""The QAP at a point in Python integers, on top of domain_ref.py (and, for the mixed 2^a 5^b sizes, of the fact that libfqfft
builds them as a basic domain over get_root_of_unity(m), which domain_ref.root_of_unity knows).

What it models (paths relative to the reference tree):
* evaluate_all_lagrange_polynomials(t): depends/libfqfft/libfqfft/evaluation_domain/domains/basic_radix2_domain_aux.tcc:333-395,
  extended_radix2_domain.tcc:120-139, step_radix2_domain.tcc:189-214 -- `lagrange_fast`, the closed forms, with the reference's
  rule for a t inside a subgroup (the indicator vector of the matching index, the outer formulas running on it);
* the same values by definition, prod_{j != i} (t - x_j) / (x_i - x_j) over domain_ref.elements -- `lagrange_def`, O(m^2), for m <= 64;
* compute_vanishing_polynomial(t) -- `vanishing`;
* r1cs_to_qap_instance_map_with_evaluation (libsnark/reductions/r1cs_to_qap/r1cs_to_qap.tcc:110-159) -- `instance_map`.

Integers are plain residues in [0, r), not Montgomery forms; domain_ref.from_wire / to_wire convert.  tests/golden/qap/ holds what
the reference's own code computes (tools/mint_qap.sh); tests/test_qap_cpu.py compares this model with every record of it.
"""
import hashlib
import json
import os

import numpy as np

import domain_ref as D

MIXED = D.MIXED
DEF_LIMIT = 64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qap")
KIND_CODE = {D.BASIC: 0, D.EXTENDED: 1, D.STEP: 2, D.MIXED: 3}      # MNT753_DOMAIN_*


def _dkind(kind):
    """a mixed domain is libfqfft's basic domain at a size 2^a 5^b"""
    return D.BASIC if kind == MIXED else kind


def vanishing(curve, kind, m, t):
    return D.vanishing(curve, _dkind(kind), m, t)


def lagrange_def(curve, kind, m, t):
    """L_i(t) by definition"""
    assert m <= DEF_LIMIT
    r = D.MODULUS[curve]
    xs = D.elements(curve, _dkind(kind), m)
    out = []
    for i, xi in enumerate(xs):
        num = den = 1
        for j, xj in enumerate(xs):
            if j != i:
                num = num * (t - xj) % r
                den = den * (xi - xj) % r
        out.append(num * pow(den, -1, r) % r)
    return out


def batch_inverse(vals, r):
    """Montgomery's simultaneous inversion; every value non-zero"""
    pre, acc = [], 1
    for v in vals:
        pre.append(acc)
        acc = acc * v % r
    inv = pow(acc, -1, r)
    out = [0] * len(vals)
    for i in range(len(vals) - 1, -1, -1):
        out[i] = inv * pre[i] % r
        inv = inv * vals[i] % r
    return out


def _subgroup(curve, n, t):
    """_basic_radix2_evaluate_all_lagrange_polynomials(n, t)"""
    r = D.MODULUS[curve]
    if n == 1:
        return [1]
    omega = D.root_of_unity(curve, n)
    roots, x = [], 1
    for _ in range(n):
        roots.append(x)
        x = x * omega % r
    if pow(t, n, r) == 1:
        return [1 if w == t else 0 for w in roots]
    l = (pow(t, n, r) - 1) * pow(n, -1, r) % r
    inv = batch_inverse([(t - w) % r for w in roots], r)
    return [l * w % r * d % r for w, d in zip(roots, inv)]


def lagrange_fast(curve, kind, m, t):
    r = D.MODULUS[curve]
    if kind in (D.BASIC, MIXED):
        return _subgroup(curve, m, t)
    if kind == D.EXTENDED:
        small = m // 2
        shift = D.G * D.G % r
        t0, t1 = _subgroup(curve, small, t), _subgroup(curve, small, t * pow(shift, -1, r) % r)
        ts, ss = pow(t, small, r), pow(shift, small, r)
        one_over_denom = pow(ss - 1, -1, r)
        c0, c1 = (ts - ss) * (-one_over_denom) % r, (ts - 1) * one_over_denom % r
        return [v * c0 % r for v in t0] + [v * c1 % r for v in t1]
    big, small = D.step_split(m)
    omega = D.root_of_unity(curve, 1 << D.clog2(m))
    inner_big, inner_small = _subgroup(curve, big, t), _subgroup(curve, small, t * pow(omega, -1, r) % r)
    os_ = pow(omega, small, r)
    l0 = (pow(t, small, r) - os_) % r
    step = pow(omega * omega % r, small, r)
    elts, e = [], 1
    for _ in range(big):
        elts.append((e - os_) % r)
        e = e * step % r
    inv = batch_inverse(elts, r)
    l1 = (pow(t, big, r) - 1) * pow(pow(omega, big, r) - 1, -1, r) % r
    return [v * l0 % r * d % r for v, d in zip(inner_big, inv)] + [l1 * v % r for v in inner_small]


def lagrange(curve, kind, m, t):
    return lagrange_def(curve, kind, m, t) if m <= DEF_LIMIT else lagrange_fast(curve, kind, m, t)


def instance_map(curve, num_inputs, nc, num_variables, mats, u, t, dm):
    """-> (At, Bt, Ct, Ht): mats = three (row_ptr, col, coeff integers); u = the dm Lagrange coefficients at t"""
    r = D.MODULUS[curve]
    out = []
    for which, (rp, col, cf) in enumerate(mats):
        v = [0] * (num_variables + 1)
        if which == 0:
            for i in range(num_inputs + 1):
                v[i] = u[nc + i]
        for row in range(nc):
            for k in range(int(rp[row]), int(rp[row + 1])):
                v[int(col[k])] = (v[int(col[k])] + u[row] * cf[k]) % r
        out.append(v)
    ht, x = [], 1
    for _ in range(dm + 1):
        ht.append(x)
        x = x * t % r
    return out[0], out[1], out[2], ht


# ---- the fixture (tests/golden/qap, tools/mint_qap.sh) --------------------------------------------------------------------------------
def index():
    with open(os.path.join(GOLDEN, "index.json")) as f:
        return json.load(f)


def lagrange_records(entry):
    """-> [(label, t words [12], Zt words [12], u words [k, 12], sample indices or None, sha256 of the full vector)] of one index entry"""
    raw = np.fromfile(os.path.join(GOLDEN, entry["file"]), dtype="<u8").reshape(-1, 12)
    idx = entry.get("sample_indices")
    per = 2 + (len(idx) if idx else entry["m"])
    assert raw.shape[0] == per * len(entry["t"])
    out = []
    for k, label in enumerate(entry["t"]):
        rec = raw[k * per:(k + 1) * per]
        out.append((label, rec[0].copy(), rec[1].copy(), rec[2:].copy(), idx, entry["u_sha256"][k]))
    return out


def qap_record(entry):
    """-> (t words, At, Bt, Ct, Ht, Zt) word arrays of one instance-map entry"""
    raw = np.fromfile(os.path.join(GOLDEN, entry["file"]), dtype="<u8").reshape(-1, 12)
    nv, dm = entry["num_variables"] + 1, entry["m"]
    assert raw.shape[0] == 3 * nv + dm + 2
    t = np.fromfile(os.path.join(GOLDEN, entry["t_file"]), dtype="<u8")
    return t, raw[:nv], raw[nv:2 * nv], raw[2 * nv:3 * nv], raw[3 * nv:3 * nv + dm + 1], raw[3 * nv + dm + 1]


def sha256_words(words):
    return hashlib.sha256(np.ascontiguousarray(words, dtype="<u8").tobytes()).hexdigest()
