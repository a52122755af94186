"""The flipped ate pairing of MNT4753 / MNT6753 and the Groth16 check in Python integers.

Written from the formulas of the reference's libff (depends/libff/libff/algebra/curves/mnt753/mnt{4,6}753/mnt*_pairing.cpp:
doubling_step_for_flipped_miller_loop, mixed_addition_step_for_flipped_miller_loop, ate_precompute_G2, ate_miller_loop,
final_exponentiation; fields fp4.tcc / fp6_2over3.tcc) and of libsnark's r1cs_gg_ppzksnark_online_verifier_weak_IC.  Nothing here is
the project's arithmetic: F elements are tuples of residues (tools/pyref.py), a tower element is a pair (c0, c1) of them.

Every constant follows from the two moduli of tools/mnt753_params.py:
  loop count |q - r| and its sign (q < r), w0 = Phi_k(q) / r - q, w1 = 1, the twist u, and the Frobenius constants
  gamma_i^j with gamma_i = NR^((q^i - 1) / k): an element is sum_j a_j w^j over Fq with w^2 = u, w^k = NR (j = half + 2 * component),
  and its q^i-th power is sum_j a_j gamma_i^j w^j.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pyref  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
VK_DIRS = ["g16_mnt4", "g16_mnt6"] + [f"keygen_mnt{c}_{t}" for c in (4, 6) for t in ("cut21", "full")]


def constants(curve):
    """-> dict of the derived pairing constants of one curve (plain integers)"""
    C = pyref.Curve(curve)
    q, r, k = C.q, C.r, 2 * C.deg
    phi = q * q + 1 if k == 4 else q * q - q + 1
    assert phi % r == 0
    w0 = phi // r - q
    gamma = [pow(C.nr, (q ** i - 1) // k, q) for i in range(k)]
    return {"q": q, "r": r, "k": k, "deg": C.deg, "nr": C.nr, "phi": phi, "loop_count": abs(q - r), "loop_neg": q < r,
            "w0_abs": abs(w0), "w0_neg": w0 < 0, "w1": 1, "gamma": gamma,
            "frob": [[pow(g, j, q) for j in range(k)] for g in gamma]}


class Pairing:
    def __init__(self, curve):
        self.curve = curve
        self.C = C = pyref.Curve(curve)
        self.K = constants(curve)
        self.deg, self.k, self.q = C.deg, 2 * C.deg, C.q
        self.twist = (0, 1) if C.deg == 2 else (0, 1, 0)
        self.twist_inv = C.f_inv(self.twist)
        self.f_one = C.f_one(self.twist)
        self.f_zero = C.f_zero(self.twist)

    # ---- F helpers ---------------------------------------------------------------------------------
    def f_mul_by_u(self, x):
        return ((self.C.nr * x[-1]) % self.q,) + tuple(x[:-1])

    def f_sqr(self, x):
        return self.C.f_mul(x, x)

    def f_embed(self, c):
        return (c % self.q,) + (0,) * (self.deg - 1)

    # ---- the tower F[v] / (v^2 - u) -------------------------------------------------------------------
    def one(self):
        return (self.f_one, self.f_zero)

    def mul(self, a, b):
        C = self.C
        v0, v1 = C.f_mul(a[0], b[0]), C.f_mul(a[1], b[1])
        s = C.f_mul(C.f_add(a[0], a[1]), C.f_add(b[0], b[1]))
        return (C.f_add(v0, self.f_mul_by_u(v1)), C.f_sub(C.f_sub(s, v0), v1))

    def sqr(self, a):
        return self.mul(a, a)

    def conj(self, a):
        """unitary inverse"""
        return (a[0], self.C.f_neg(a[1]))

    def inv(self, a):
        C = self.C
        n = C.f_sub(self.f_sqr(a[0]), self.f_mul_by_u(self.f_sqr(a[1])))
        ni = C.f_inv(n)
        return (C.f_mul(a[0], ni), C.f_neg(C.f_mul(a[1], ni)))

    def frobenius(self, a, i):
        fr, q = self.K["frob"][i % self.k], self.q
        return tuple(tuple(a[h][c] * fr[h + 2 * c] % q for c in range(self.deg)) for h in range(2))

    def pow(self, a, e):
        res = self.one()
        for bit in bin(e)[2:]:
            res = self.sqr(res)
            if bit == "1":
                res = self.mul(res, a)
        return res

    # ---- G2 precomputation ------------------------------------------------------------------------------
    def dbl_step(self, R):
        C, S = self.C, self.f_sqr
        add, sub, mul = C.f_add, C.f_sub, C.f_mul
        X, Y, Z, T = R
        A, B, Cc = S(T), S(X), S(Y)
        D = S(Cc)
        E = sub(sub(S(add(X, Cc)), B), D)
        F = add(add(add(B, B), B), mul(C.a2, A))
        G = S(F)
        E2 = add(E, E)
        X3 = sub(G, add(E2, E2))
        D8 = add(D, D); D8 = add(D8, D8); D8 = add(D8, D8)
        Y3 = sub(mul(F, sub(E2, X3)), D8)
        Z3 = sub(sub(S(add(Y, Z)), Cc), S(Z))
        T3 = S(Z3)
        H = sub(sub(S(add(Z3, T)), T3), A)
        C4 = add(Cc, Cc); C4 = add(C4, C4)
        J = sub(sub(S(add(F, T)), G), A)
        L = sub(sub(S(add(F, X)), G), B)
        return (X3, Y3, Z3, T3), (H, C4, J, L)

    def add_step(self, bx, by, by2, R):
        C, S = self.C, self.f_sqr
        add, sub, mul = C.f_add, C.f_sub, C.f_mul
        X1, Y1, Z1, T1 = R
        B = mul(bx, T1)
        D = mul(sub(sub(S(add(by, Z1)), by2), T1), T1)
        H = sub(B, X1)
        I = S(H)
        E = add(I, I); E = add(E, E)
        J = mul(H, E)
        V = mul(X1, E)
        Y2 = add(Y1, Y1)
        L1 = sub(D, Y2)
        X3 = sub(sub(S(L1), J), add(V, V))
        Y3 = sub(mul(L1, sub(V, X3)), mul(Y2, J))
        Z3 = sub(sub(S(add(Z1, H)), T1), I)
        return (X3, Y3, Z3, S(Z3)), (L1, Z3)

    def loop_bits(self):
        return bin(self.K["loop_count"])[3:]     # below the most significant bit, high to low

    def precompute_g2(self, Q):
        C = self.C
        qx, qy = Q
        out = {"QX_over_twist": C.f_mul(qx, self.twist_inv), "QY_over_twist": C.f_mul(qy, self.twist_inv), "dbl": [], "add": []}
        qy2 = self.f_sqr(qy)
        R = (qx, qy, self.f_one, self.f_one)
        for bit in self.loop_bits():
            R, dc = self.dbl_step(R)
            out["dbl"].append(dc)
            if bit == "1":
                R, ac = self.add_step(qx, qy, qy2, R)
                out["add"].append(ac)
        if self.K["loop_neg"]:
            zi = C.f_inv(R[2])
            zi2 = self.f_sqr(zi)
            zi3 = C.f_mul(zi2, zi)
            mx, my = C.f_mul(R[0], zi2), C.f_neg(C.f_mul(R[1], zi3))
            R, ac = self.add_step(mx, my, self.f_sqr(my), R)
            out["add"].append(ac)
        return out

    # ---- Miller loop ---------------------------------------------------------------------------------------
    def miller_loop(self, P, prec):
        C = self.C
        add, sub, mul, neg = C.f_add, C.f_sub, C.f_mul, C.f_neg
        px_t, py_t = mul(self.f_embed(P[0]), self.twist), mul(self.f_embed(P[1]), self.twist)
        l1c = sub(self.f_embed(P[0]), prec["QX_over_twist"])
        qyt = prec["QY_over_twist"]

        def g_rq(ac):
            return (mul(ac[1], py_t), neg(add(mul(qyt, ac[1]), mul(l1c, ac[0]))))
        f, ai = self.one(), 0
        for di, bit in enumerate(self.loop_bits()):
            H, C4, J, L = prec["dbl"][di]
            g = (add(sub(neg(C4), mul(J, px_t)), L), mul(H, py_t))
            f = self.mul(self.sqr(f), g)
            if bit == "1":
                f = self.mul(f, g_rq(prec["add"][ai]))
                ai += 1
        if self.K["loop_neg"]:
            f = self.inv(self.mul(f, g_rq(prec["add"][ai])))
        return f

    def miller(self, P, Q):
        return self.miller_loop(P, self.precompute_g2(Q))

    # ---- final exponentiation ----------------------------------------------------------------------------------
    def first_chunk(self, e, e_inv):
        if self.k == 4:
            return self.mul(self.frobenius(e, 2), e_inv)
        t = self.mul(self.frobenius(e, 3), e_inv)
        return self.mul(self.frobenius(t, 1), t)

    def final_exponentiation(self, f):
        fi = self.inv(f)
        a, b = self.first_chunk(f, fi), self.first_chunk(fi, f)
        w1 = self.frobenius(a, 1)
        w0 = self.pow(b if self.K["w0_neg"] else a, self.K["w0_abs"])
        return self.mul(w1, w0)

    def reduced_pairing(self, P, Q):
        """P, Q affine (pyref points).  The identity in either argument gives one (the device's convention; libff's value there is
        not meaningful)."""
        if P is None or Q is None:
            return self.one()
        return self.final_exponentiation(self.miller(P, Q))

    # ---- wire form --------------------------------------------------------------------------------------------
    def gt_to_words(self, g):
        return np.array(self.C.coord_to_words(g[0]) + self.C.coord_to_words(g[1]), dtype=np.uint64)

    def gt_from_words(self, w):
        d = self.deg
        w = [int(v) for v in w]
        return (self.C.coord_from_words(w[:12 * d], d), self.C.coord_from_words(w[12 * d:24 * d], d))

    def pair_words(self, p_words, q_words):
        """wire-format affine G1 / G2 points -> GT wire words"""
        P = self.C.affine_from_words([int(v) for v in p_words], 1)
        Q = self.C.affine_from_words([int(v) for v in q_words], 2)
        return self.gt_to_words(self.reduced_pairing(P, Q))

    # ---- Groth16 (r1cs_gg_ppzksnark_online_verifier_weak_IC) -----------------------------------------------------
    def groth16_verify(self, alpha_beta, delta, abc, proof, inputs):
        """alpha_beta: GT; delta: G2 point; abc: num_inputs + 1 G1 points; proof: (A, B, C); inputs: integers.  The reference's form:
        FE(ML(A, B) * unitary_inverse(ML(acc, G2::one()) * ML(C, delta))) == alpha_beta."""
        C = self.C
        A, B, Cp = proof
        acc = abc[0]
        for x, pt in zip(inputs, abc[1:]):
            acc = C.add(acc, C.mul(x % C.r, pt, 1), 1)
        qap = self.miller(A, B)
        rest = self.mul(self.miller(acc, C.gen(2)), self.miller(Cp, delta))
        return self.final_exponentiation(self.mul(qap, self.conj(rest))) == alpha_beta


# ---- fixtures -------------------------------------------------------------------------------------------------------
def dir_curve(name):
    return 0 if "mnt4" in name else 1


def vk_head(name):
    """the GT element at the head of tests/golden/<name>/vk.txt, as wire words"""
    n = 2 * (2 if dir_curve(name) == 0 else 3) * 96
    with open(os.path.join(GOLDEN, name, "vk.txt"), "rb") as f:
        return np.frombuffer(f.read(n), dtype="<u8").astype(np.uint64)


def alpha_beta_words(name):
    """alpha_g1, beta_g2 of tests/golden/<name>/keys.bin (alpha_g1 | beta_g1 | beta_g2 | delta_g1 | delta_g2), wire words"""
    curve = dir_curve(name)
    w2 = 24 * (2 if curve == 0 else 3)
    keys = np.fromfile(os.path.join(GOLDEN, name, "keys.bin"), dtype="<u8").astype(np.uint64)
    assert keys.size == 3 * 24 + 2 * w2
    return keys[:24], keys[48:48 + w2]


def delta_words(name):
    keys = np.fromfile(os.path.join(GOLDEN, name, "keys.bin"), dtype="<u8").astype(np.uint64)
    w2 = 24 * (2 if dir_curve(name) == 0 else 3)
    return keys[72 + w2:72 + 2 * w2]


def serialize_vk(curve, gt_words, delta_words_, abc_words):
    """The reference's vk.txt under BINARY_OUTPUT, MONTGOMERY_OUTPUT and NO_PT_COMPRESSION: GT | '0' delta_g2 | '0' ABC[0] | the
    sparse_vector header of the rest (domain size, number of indices, the indices, number of values; each followed by a newline) and
    '0' ABC[j] for j >= 1.  abc_words: [num_inputs + 1, 24]."""
    abc = np.asarray(abc_words, dtype="<u8").reshape(-1, 24)
    n = abc.shape[0] - 1
    raw = lambda a: np.asarray(a, dtype="<u8").tobytes()
    out = raw(gt_words) + b"0" + raw(delta_words_) + b"0" + raw(abc[0])
    out += b"%d\n%d\n" % (n, n) + b"".join(b"%d\n" % i for i in range(n)) + b"%d\n" % n
    for j in range(1, n + 1):
        out += b"0" + raw(abc[j])
    return out
