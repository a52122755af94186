"""Folded Groth16 verification in Python integers, on top of tests/pairing_ref.py and tests/subgroup_ref.py.

For proofs (A_i, B_i, C_i) with inputs x_i and coefficients 0 < rho_i < 2^128:
    U_i = rho_i A_i,  T = sum rho_i C_i,  rho = sum rho_i mod r,  c_j = sum_i rho_i x_ij mod r,  S = rho ABC[0] + sum_j c_j ABC[j + 1],
    F = prod_i ML(U_i, B_i)                                  (unreduced Miller values)
    accept  <=>  FE(F ML(-S, G2::one()) ML(-T, delta)) == e(alpha, beta)^rho.
Nothing here is the project's arithmetic: points are pyref's affine tuples, the group law is pyref's complete one, the Miller loop
and the tower are pairing_ref's."""
import functools
import os

import numpy as np

import pairing_ref as PR
import pyref
import subgroup_ref as S


@functools.lru_cache(maxsize=None)
def model(curve):
    return PR.Pairing(curve)


@functools.lru_cache(maxsize=None)
def _miller(curve, P, Q):
    return model(curve).miller(P, Q)


def w2(curve):
    return 24 * (2 if curve == 0 else 3)


class Key:
    """alpha_beta: the GT element e(alpha, beta); delta: a G2 point; abc: num_inputs + 1 G1 points"""

    def __init__(self, curve, alpha_beta, delta, abc):
        self.curve, self.alpha_beta, self.delta, self.abc = curve, alpha_beta, delta, list(abc)


@functools.lru_cache(maxsize=None)
def g16_words(curve):
    """the committed g16 fixture in wire words -> alpha_g1, beta_g2, delta_g2, ABC (2 points), the proof, its one public input"""
    name = f"g16_mnt{4 if curve == 0 else 6}"
    path = lambda f: os.path.join(PR.GOLDEN, name, f)
    alpha, beta = PR.alpha_beta_words(name)
    raw = open(path("vk.txt"), "rb").read()
    pos = 8 * w2(curve) + 1 + 8 * w2(curve)                                # GT | '0' delta
    abc0 = np.frombuffer(raw[pos + 1:pos + 193], dtype="<u8").astype(np.uint64)
    pos += 193
    assert raw[pos:pos + 9] == b"1\n1\n0\n1\n0"
    abc1 = np.frombuffer(raw[pos + 9:pos + 9 + 192], dtype="<u8").astype(np.uint64)
    proof = np.fromfile(path("full.bin"), dtype="<u8").astype(np.uint64)
    inp = np.fromfile(path("input.bin"), dtype="<u8", count=24).astype(np.uint64)[12:]
    return alpha, beta, PR.delta_words(name), np.concatenate([abc0, abc1]), proof, inp


@functools.lru_cache(maxsize=None)
def g16_key(curve):
    C = model(curve).C
    _, _, delta, abc, _, _ = g16_words(curve)
    gt = model(curve).gt_from_words(PR.vk_head(f"g16_mnt{4 if curve == 0 else 6}"))
    return Key(curve, gt, C.affine_from_words([int(v) for v in delta], 2), [C.affine_from_words([int(v) for v in abc[24 * j:24 * j + 24]], 1) for j in range(2)])


def proof_from_words(curve, w):
    C = model(curve).C
    w = [int(v) for v in w]
    return (C.affine_from_words(w[:24], 1), C.affine_from_words(w[24:24 + w2(curve)], 2), C.affine_from_words(w[24 + w2(curve):], 1))


def proof_to_words(curve, proof):
    C = model(curve).C
    return np.array(C.affine_to_words(proof[0], 1) + C.affine_to_words(proof[1], 2) + C.affine_to_words(proof[2], 1), dtype=np.uint64)


def rerandomised(curve, proof, k):
    """(k A, k^-1 B, C): another valid proof of the same statement"""
    C = model(curve).C
    return (C.mul(k % C.r, proof[0], 1), C.mul(pow(k, -1, C.r), proof[1], 2), proof[2])


def coefficient_words(rhos):
    return np.array([(int(v) >> (64 * k)) & (2 ** 64 - 1) for v in rhos for k in range(2)], dtype=np.uint64).reshape(-1, 2)


def g1_parts(key, proofs, inputs, rhos):
    """-> U (list), T, S, rho, c (list): the G1 side.  Equal C_i are scaled once by the sum of their coefficients."""
    C = model(key.curve).C
    assert all(0 < k < 2 ** 128 for k in rhos)
    U = [C.mul(k, p[0], 1) for k, p in zip(rhos, proofs)]
    by_c = {}
    for k, p in zip(rhos, proofs):
        by_c[p[2]] = by_c.get(p[2], 0) + k
    T = None
    for pt, k in by_c.items():
        T = C.add(T, C.mul(k % C.r, pt, 1), 1)
    rho = sum(rhos) % C.r
    c = [sum(k * x[j] for k, x in zip(rhos, inputs)) % C.r for j in range(len(key.abc) - 1)]
    Sp = C.mul(rho, key.abc[0], 1)
    for cj, pt in zip(c, key.abc[1:]):
        Sp = C.add(Sp, C.mul(cj, pt, 1), 1)
    return U, T, Sp, rho, c


def product(curve, values):
    P = model(curve)
    f = P.one()
    for v in values:
        f = P.mul(f, v)
    return f


def parts(key, proofs, inputs, rhos):
    """-> dict U, T, S, rho, c, F: F the product of the unreduced Miller values of the pairs (U_i, B_i)"""
    U, T, Sp, rho, c = g1_parts(key, proofs, inputs, rhos)
    F = product(key.curve, [_miller(key.curve, u, p[1]) for u, p in zip(U, proofs)])
    return {"U": U, "T": T, "S": Sp, "rho": rho, "c": c, "F": F}


def verdict(key, pt):
    """the folded equation on parts(); a pair with the identity is one"""
    P = model(key.curve)
    C = P.C
    f = pt["F"]
    if pt["S"] is not None:
        f = P.mul(f, _miller(key.curve, C.neg(pt["S"]), C.gen(2)))
    if pt["T"] is not None:
        f = P.mul(f, _miller(key.curve, C.neg(pt["T"]), key.delta))
    return P.final_exponentiation(f) == P.pow(key.alpha_beta, pt["rho"])


def accepts(key, proofs, inputs, rhos):
    return verdict(key, parts(key, proofs, inputs, rhos))


def status(curve, proof):
    """0, 1 (a point off its curve or the identity) or 3 (B on the twist, outside G2)"""
    C = model(curve).C
    A, B, Cp = proof
    if A is None or B is None or Cp is None or not (C.on_curve(A, 1) and C.on_curve(B, 2) and C.on_curve(Cp, 1)):
        return 1
    return 0 if S.in_subgroup(curve, B) else 3


def g1_words(curve, pt):
    return np.array(model(curve).C.affine_to_words(pt, 1), dtype=np.uint64)


def fr_words(curve, x):
    return np.array(model(curve).C.fr_to_words(x), dtype=np.uint64)
