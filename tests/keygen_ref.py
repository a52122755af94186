"""The scalar side of the Groth16 generator in Python integers, on top of qap_ref.py: what r1cs_gg_ppzksnark_generator
(libsnark/zk_proof_systems/ppzksnark/r1cs_gg_ppzksnark/r1cs_gg_ppzksnark.tcc:212-362) computes before it touches a group, for given
t, alpha, beta, delta.

* `touched` / `swap_rule`: swap_AB_if_beneficial (libsnark/relations/constraint_satisfaction_problems/r1cs/r1cs.tcc:194-243);
* `combine`: the ABC | Lt vector (:252-274) -- entries 0 .. num_inputs are ABC, the rest is Lt;
* `h_scalars`: the scalars of the H query, t^i Z(t) / delta for i < m_d - 1 (:281, :331);
* `key_scalars`: all of it for one system, with the query densities (:230-244).

Integers are plain residues in [0, r).  tests/golden/keygen_mnt{4,6}_{full,cut21}/ hold what the reference's own functions make
of the same inputs (tools/mint_keygen.sh); tests/test_keygen_cpu.py multiplies the generators by these scalars with the CPU oracle and
compares with the fixtures' bytes.
"""
import json
import os

import numpy as np

import domain_ref as D
import qap_ref as Q

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CLASS_KIND = {"basic_radix2_domain": D.BASIC, "extended_radix2_domain": D.EXTENDED, "step_radix2_domain": D.STEP}
FIXTURES = [(curve, tag) for curve in (0, 1) for tag in ("full", "cut21")]
QUERY_FILES = ("params.bin", "keys.bin", "vk_elements.bin", "r1cs.bin")


def fixture_dir(curve, tag):
    return os.path.join(GOLDEN, f"keygen_mnt{4 if curve == 0 else 6}_{tag}")


def fixture_id(f):
    return f"mnt{4 if f[0] == 0 else 6}-{f[1]}"


def index(curve, tag):
    with open(os.path.join(fixture_dir(curve, tag), "index.json")) as f:
        return json.load(f)


def randomness(curve, tag):
    """-> t, alpha, beta, delta (12 words each) and the G1 generator (24 words) of randomness.bin"""
    raw = np.fromfile(os.path.join(fixture_dir(curve, tag), "randomness.bin"), dtype="<u8").astype(np.uint64)
    assert raw.size == 4 * 12 + 24
    return raw[0:12], raw[12:24], raw[24:36], raw[36:48], raw[48:72]


def aff_words(curve, group):
    return 24 * (1 if group == 1 else (2 if curve == 0 else 3))


def touched(num_variables, mat):
    """the variables a term of the matrix names, whatever its coefficient"""
    rp, col, _ = mat
    seen = [False] * (num_variables + 1)
    for c in col[:int(rp[-1])]:
        seen[int(c)] = True
    return sum(seen)


def swap_rule(num_variables, mats):
    """-> (swapped, the matrices as the generator uses them): a and b change roles if b touches STRICTLY more variables"""
    a, b = touched(num_variables, mats[0]), touched(num_variables, mats[1])
    return (True, [mats[1], mats[0], mats[2]]) if b > a else (False, list(mats))


def combine(curve, at, bt, ct, num_inputs, alpha, beta, delta_inv):
    r = D.MODULUS[curve]
    return [(beta * a + alpha * b + c) % r * (1 if i <= num_inputs else delta_inv) % r for i, (a, b, c) in enumerate(zip(at, bt, ct))]


def h_scalars(curve, t, dm, zt, delta_inv):
    r = D.MODULUS[curve]
    coeff, out, x = zt * delta_inv % r, [], 1
    for _ in range(dm - 1):
        out.append(x * coeff % r)
        x = x * t % r
    return out


def key_scalars(curve, num_inputs, num_variables, nc, mats, kind, dm, t, alpha, beta, delta):
    """mats: three (row_ptr, col, coeff integers) as given (before the swap).  -> dict: swapped, the scalars of A (= At), B (= Bt),
    ABC, L and H, the densities."""
    r = D.MODULUS[curve]
    swapped, used = swap_rule(num_variables, mats)
    u = Q.lagrange(curve, kind, dm, t)
    at, bt, ct, _ = Q.instance_map(curve, num_inputs, nc, num_variables, used, u, t, dm)
    zt = Q.vanishing(curve, kind, dm, t)
    dinv = pow(delta, -1, r)
    comb = combine(curve, at, bt, ct, num_inputs, alpha, beta, dinv)
    return {"swapped": swapped, "A": at, "B": bt, "ABC": comb[:num_inputs + 1], "L": comb[num_inputs + 1:], "H": h_scalars(curve, t, dm, zt, dinv),
            "non_zero_At": sum(1 for v in at if v), "non_zero_Bt": sum(1 for v in bt if v), "Zt": zt}


def read_r1cs(path):
    """r1cs.bin -> num_inputs, m, nc, [(row_ptr, col, coeff words [nnz, 12])] x 3"""
    raw = np.fromfile(path, dtype=np.uint8)
    num_inputs, m, nc = (int(v) for v in raw[:24].view("<u8"))
    pos, mats = 24, []
    for _ in range(3):
        rp = raw[pos:pos + 8 * (nc + 1)].view("<u8").astype(np.uint64); pos += 8 * (nc + 1)
        nnz = int(rp[nc])
        col = raw[pos:pos + 4 * nnz].view("<u4").astype(np.uint32); pos += 4 * nnz
        cf = raw[pos:pos + 96 * nnz].view("<u8").astype(np.uint64).reshape(nnz, 12); pos += 96 * nnz
        mats.append((rp, col, cf))
    assert pos == raw.size
    return num_inputs, m, nc, mats


def split_params(curve, raw, num_inputs):
    """params.bin bytes -> d, m, {A, B1, B2, L, H: uint64 words [n, affine words]}"""
    words = np.frombuffer(raw, dtype="<u8").astype(np.uint64)
    d, m = int(words[0]), int(words[1])
    w1, w2 = aff_words(curve, 1), aff_words(curve, 2)
    out, pos = {}, 2
    for name, n, w in (("A", m + 1, w1), ("B1", m + 1, w1), ("B2", m + 1, w2), ("L", m - num_inputs, w1), ("H", d, w1)):
        out[name] = words[pos:pos + n * w].reshape(n, w)
        pos += n * w
    assert pos == words.size
    return d, m, out
