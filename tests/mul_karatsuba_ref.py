"""Reference for the signed product with a Karatsuba product half (fp_mul_s_k / fp_mul_s_ip_k, csrc/fp753.hip.h): the raw ops
FR_MUL_S_K / FR_MUL_S_IP_K of csrc/field_raw_ops.hip.h, appended behind FR_INV_GROUP.  The representation helpers and the exact Montgomery
value are tests/field_raw_ref.py's; this module adds the two op codes, the operand set of the products' contract and the expected limbs.

Contract (stated above fp_mul_s_k): one operand N with limbs 0..25 in [0, 2^28) and limb 26 in (-2^26, 2^28), the other R with
|limb| < 2^29.  The result is fp_mul_s's limb for limb: limbs 0..25 of (a b + m p) / R' in [0, 2^28), the rest signed in limb 26.
"""
import os
import re

import numpy as np

import field_raw_ref as F

OP_MUL_S_K, OP_MUL_S_IP_K = 25, 26      # FR_MUL_S_K, FR_MUL_S_IP_K (header_codes() reads them back from the header)
N_MAX, R_MAX, TOP_MIN = (1 << 28) - 1, (1 << 29) - 1, -(1 << 26) + 1
H = 14                                   # limbs of the low half


def header_codes():
    """{enumerator: value} of FieldRawOp in csrc/field_raw_ops.hip.h, by the rules of a C enum"""
    hdr = os.path.join(F.ROOT, "snark-challenge-prover-reference_amd", "csrc", "field_raw_ops.hip.h")
    body = re.search(r"enum FieldRawOp : int \{(.*?)\n\};", open(hdr).read(), re.S).group(1)
    codes, nxt = {}, 0
    for name, val in re.findall(r"^\s*(FR_\w+)(?:\s*=\s*(\d+))?\s*,?", body, re.M):
        nxt = int(val) if val else nxt
        codes[name] = nxt
        nxt += 1
    return codes


def halves(low, high):
    return [low] * H + [high] * (F.NL - H)


def signed(l):
    return [F.s32(int(x)) for x in l]


def edge_pairs(p):
    """[(a, b)] signed limb lists: every N edge against every R edge, in both argument orders.  N: every limb at 0 and at 2^28 - 1, the
    halves at opposite extremes, the same with the top limb at its negative end, the values 0, p, 2p - 1; R: every limb at 0, 2^28 - 1,
    +-(2^29 - 1), the halves at opposite extremes (the patterns that maximise the middle term), alternating signs, the three values"""
    vals = [signed(F.to_limbs(v)) for v in (0, p, 2 * p - 1)]
    N = [halves(lo, hi) for lo in (0, N_MAX) for hi in (0, N_MAX)]
    N += [n[:-1] + [TOP_MIN] for n in N[:4]] + vals
    R = [halves(c, c) for c in (0, N_MAX, R_MAX, -R_MAX)]
    R += [halves(R_MAX, -R_MAX), halves(-R_MAX, R_MAX), halves(R_MAX, 0), halves(0, R_MAX), halves(-R_MAX, 0), halves(0, -R_MAX)]
    R += [[R_MAX if i & 1 else -R_MAX for i in range(F.NL)], [-R_MAX if i & 1 else R_MAX for i in range(F.NL)]] + vals
    return [(n, r) for n in N for r in R] + [(r, n) for n in N for r in R]


def random_pairs(p, rng, n):
    """n pairs inside the contract: any limbs in range, or a lazy element (as a product output: small signed top limb) against the
    limb-wise difference of two lazy elements -- the forward sweep's operands; either argument order"""
    out = []
    for t in range(n):
        if t % 2:
            a = [rng.randint(0, N_MAX) for _ in range(F.NL - 1)] + [rng.randint(TOP_MIN, N_MAX)]
            b = [rng.randint(-R_MAX, R_MAX) for _ in range(F.NL)]
        else:
            a = signed(F.to_limbs(rng.randrange(-3 * p // 10, 13 * p // 10)))
            b = [x - y for x, y in zip(F.to_limbs(F.rand_lazy(p, rng)), F.to_limbs(F.rand_lazy(p, rng)))]
        out.append((a, b) if t % 4 < 2 else (b, a))
    return out


def records(pairs):
    """operands x0 = a, x1 = b of every pair, as the (n, IN_WORDS) array the hooks take"""
    return F.records_array([[F.raw_limbs(a), F.raw_limbs(b)] for a, b in pairs])


def expected_limbs(pairs, p):
    """the limbs of a b 2^-756 as fp_mul_s leaves them, from Python integers: (n, NL) uint32"""
    raw = lambda l: sum(x << (F.LB * i) for i, x in enumerate(l))
    return np.array([F.to_limbs(F.mont(raw(a), raw(b), p)) for a, b in pairs], dtype=np.uint64).astype(np.uint32)
