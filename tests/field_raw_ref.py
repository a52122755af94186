"""Exact reference and edge generator for the device field primitives on raw limbs (csrc/field_raw_ops.hip.h).

Pure Python integers.  A device element is 27 uint32 limbs of 28 bits, value sum limb_i 2^(28 i), Montgomery radix R' = 2^756.  The
lazy primitives of fp753.hip.h / fp_inv.hip.h take and return values outside [0, p): limb 26 may be signed ("std" value) or every limb
may be signed ("raw" value, the carry-free differences).  For every op, `cases` draws operands inside the contract stated above the
primitive and pushed to its edges, and `check` asserts three things of a result: the residue mod p, the stated value range and the
stated limb bounds.  Used by tests/test_field_raw_cpu.py (the g++ twin) and tests/test_field_raw_gpu.py (the device hook).
"""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import mnt753_params as P  # noqa: E402

NL, LB = 27, 28
MASK = (1 << LB) - 1
RB = 1 << (NL * LB)             # R' = 2^756
MODS = (P.MOD_A, P.MOD_B)       # mod 0 = modulus A, 1 = modulus B (csrc/mnt753_constants.h)
IN_WORDS, OUT_WORDS = 6 * NL, 2 * NL + 1

# op codes of field_raw_ops.hip.h (FieldRawOp)
(MUL, SQR, MUL2, MUL3, REDUCE2P, ADD, SUB, NEG, HALF, MUL_SMALL, MUL_S, SQR_S, MUL_S_IP, SQR_S_KEEP, SUB_RAW, ADDSUB_RAW, NORM,
 RAW_MAYBE_ZERO, IS_ZERO, CANON, INV, FROM_WIRE, TO_WIRE, NTT2) = range(24)
OP_NAMES = ("mul", "sqr", "mul2", "mul3", "reduce2p", "add", "sub", "neg", "half", "mul_small", "mul_s", "sqr_s", "mul_s_ip",
            "sqr_s_keep", "sub_raw", "addsub_raw", "norm", "raw_maybe_zero", "is_zero", "canon", "inv", "from_wire", "to_wire", "ntt2")
# ops whose device result may differ in representative from the host twin's (hipcc contracts fp_norm's float x * (1 / p_top) - 0.5
# into an FMA, g++ on x86-64 does not): only residue and range are required of them.  (op, k) -> True
def involves_norm(op, k):
    return op == NORM or (op == NTT2 and (k >> 2) == 2)


# ---- representations ----------------------------------------------------------------------------------------------------------
def s32(w):
    w &= 0xFFFFFFFF
    return w - (1 << 32) if w >> 31 else w


def to_limbs(v):
    """limbs 0..25 in [0, 2^28), limb 26 signed (as uint32): the representation of every non-lazy output"""
    top = v >> (LB * (NL - 1))
    assert -(1 << 31) <= top < (1 << 31), "value outside the int32 top limb"
    return [(v >> (LB * i)) & MASK for i in range(NL - 1)] + [top & 0xFFFFFFFF]


def val_std(l):
    return sum(int(l[i]) << (LB * i) for i in range(NL - 1)) + (s32(int(l[NL - 1])) << (LB * (NL - 1)))


def val_raw(l):
    return sum(s32(int(l[i])) << (LB * i) for i in range(NL))


def raw_limbs(signed):
    return [x & 0xFFFFFFFF for x in signed]


def normalised(l):
    return all(0 <= int(x) <= MASK for x in l)


def max_abs_limb(l):
    return max(abs(s32(int(x))) for x in l)


# ---- edges ---------------------------------------------------------------------------------------------------------------------
def limb_max_below(bound, limb_max=MASK):
    """largest value < bound whose limbs 0..25 are all limb_max (limb 26 takes what is left)"""
    low = sum(limb_max << (LB * i) for i in range(NL - 1))
    top = (bound - 1 - low) >> (LB * (NL - 1))
    return [limb_max] * (NL - 1) + [top]


def edge_values(p, bound, rng, n_rand=6):
    """normalised values in [0, bound): the fixed edges, random values in [p, 2p) and [0, p), the Montgomery one, limb patterns"""
    vs = [0, 1, 2, p - 1, p, p + 1, 2 * p - 2, 2 * p - 1, 3 * p, 4 * p - 1, RB % p, (RB * RB) % p, p >> 1, (p + 1) >> 1]
    vs += [rng.randrange(p, 2 * p) for _ in range(n_rand)] + [rng.randrange(p) for _ in range(n_rand)]
    vs += [val_std(limb_max_below(bound))]
    vs += [MASK << (LB * i) for i in (0, 1, 13, 25, 26)] + [(1 << 753) - 1, 1 << 752]
    out = []
    for v in vs:
        if 0 <= v < bound and v not in out:
            out.append(v)
    return out


def rand_lazy(p, rng, bound_mul=2):
    return rng.randrange(bound_mul * p) if rng.random() < 0.5 else rng.randrange(p, bound_mul * p)


def scramble(v, limb_bound, rng, push=True):
    """signed raw limbs of value v with |limb| < limb_bound: carries moved between neighbours, limbs pushed towards +-limb_bound"""
    l = [(v >> (LB * i)) & MASK for i in range(NL - 1)] + [v >> (LB * (NL - 1))]
    for i in range(NL - 1):
        lo_t = -((limb_bound - 1 + l[i]) >> LB)       # smallest t with l + t 2^28 > -limb_bound
        hi_t = (limb_bound - 1 - l[i]) >> LB          # largest t with l + t 2^28 < limb_bound
        t = (hi_t if rng.random() < 0.5 else lo_t) if push else rng.randint(lo_t, hi_t)
        if abs(l[i + 1] - t) >= limb_bound and i + 1 == NL - 1:
            t = 0
        l[i] += t << LB
        l[i + 1] -= t
    if abs(l[NL - 1]) >= limb_bound:
        return None
    assert sum(x << (LB * i) for i, x in enumerate(l)) == v
    return raw_limbs(l)


def norm_limb_bound(v, p):
    """fp_norm's limb bound for value v: |limb| < 2^30 and |limb| + 2^28 |q| < 2^31 - 2^4 for the quotient q it takes off -- the
    floor of v / p - 1/2, or one off from it within 2^-20 p of a half-integer multiple of p (the top limb alone decides)"""
    d = p >> 20
    q = max(abs((2 * (v + e) - p) // (2 * p)) for e in (-d, 0, d))
    return min(1 << 30, (1 << 31) - (1 << 4) - (q << LB))


def mul_s_prod_max(p):
    """fp_mul_s / fp_sqr_s: the largest |a_i| |b_j| with 27 |a_i| |b_j| + (2^28 - 1) sum_j p_j + 2^36 < 2^63 (a column's products,
    its reduction products, the carry in)"""
    sp = sum((p >> (LB * i)) & MASK for i in range(NL))
    return ((1 << 63) - (1 << 36) - MASK * sp - 1) // 27


def mont(a, b, p):
    """the exact value of a Montgomery product of a and b (any signs): (a b + m p) / R' with m = -a b p^-1 mod R' in [0, R')"""
    m = (-a * b * pow(p, -1, RB)) % RB
    return (a * b + m * p) // RB


# ---- cases: {k: [operand lists]} ----------------------------------------------------------------------------------------------
def cases(mod, op, rng, n_random):
    p = MODS[mod]
    E = edge_values(p, 2 * p, rng)
    L = [to_limbs(v) for v in E]
    rl = lambda: to_limbs(rand_lazy(p, rng))
    recs = {0: []}
    R = recs[0]

    def lsum(x, y):                     # limb-wise sum of two [0, 2p) values: limbs up to 2^29 - 2, value < 4p
        return [a + b for a, b in zip(x, y)]

    def lsub(x, y):                     # limb-wise difference: signed limbs, |limb| < 2^28
        return raw_limbs([s32(a) - s32(b) for a, b in zip(x, y)])

    if op in (MUL, MUL2, MUL3, ADD, SUB, SQR, NEG, CANON, IS_ZERO, INV):
        nops = {MUL: 2, MUL2: 4, MUL3: 6, ADD: 2, SUB: 2}.get(op, 1)
        if nops == 1:
            R += [[x] for x in L]
        else:
            for x in L:
                for y in L:
                    R.append([x, y] + [L[rng.randrange(len(L))] for _ in range(nops - 2)])
            R += [[L[-1]] * nops, [to_limbs(2 * p - 1)] * nops]
        R += [[rl() for _ in range(nops)] for _ in range(n_random)]
        if op == MUL:                   # a < 4p with limbs up to 2^29 (one un-normalised addition), b < p
            Lp = [to_limbs(v) for v in E if v < p]
            R += [[to_limbs(4 * p - 1), to_limbs(p - 1)], [limb_max_below(4 * p), to_limbs(p - 1)]]
            for _ in range(n_random):
                x, y = rl(), rl()
                if val_std(x) + val_std(y) < 4 * p:
                    R.append([lsum(x, y), Lp[rng.randrange(len(Lp))] if rng.random() < 0.3 else to_limbs(rng.randrange(p))])
            for x in L:
                for y in L:
                    if val_std(x) + val_std(y) < 4 * p:
                        R.append([lsum(x, y), to_limbs(p - 1)])
        if op in (IS_ZERO, CANON):      # words equal to p's in all but one limb
            for i in (0, 1, 26):
                v = to_limbs(p)
                v[i] ^= 1
                R.append([v])
        if op == INV:
            R += [[to_limbs(1 << e)] for e in range(0, 754)]
            R += [[to_limbs(w << (LB * i))] for i in range(NL) for w in (1, 3, MASK) if (w << (LB * i)) < 2 * p]
    elif op == REDUCE2P:                # normalised limbs, value < 4p
        vs = edge_values(p, 4 * p, rng) + [2 * p, 2 * p + 1, 4 * p - 1, 4 * p - 2, 2 * p - 1]
        R += [[to_limbs(v)] for v in vs] + [[limb_max_below(4 * p)]]
        R += [[to_limbs(rng.randrange(4 * p))] for _ in range(n_random)]
    elif op == HALF:                    # non-negative limbs < 2^30, value < 8p
        R += [[x] for x in L]
        R += [[limb_max_below(8 * p, (1 << 30) - 1)], [to_limbs(8 * p - 1)], [to_limbs(8 * p - 2)]]
        for _ in range(n_random):
            xs = [rl() for _ in range(rng.randint(1, 4))]
            R.append([[sum(c) for c in zip(*xs)]])
            hi = limb_max_below(8 * p, (1 << 30) - 1)
            R.append([[rng.randrange((1 << 30)) for _ in range(NL - 1)] + [rng.randrange(hi[-1] + 1)]])
    elif op == MUL_SMALL:               # a in [0, 2p), every k < 256 on the edge set, random k on random a
        recs = {k: [[x] for x in L] + [[limb_max_below(2 * p)]] for k in range(256)}
        for _ in range(n_random):
            recs[rng.randrange(256)].append([rl()])
        return recs
    elif op in (MUL_S, MUL_S_IP, SQR_S, SQR_S_KEEP):
        unary = op in (SQR_S, SQR_S_KEEP)
        for x in L:                     # differences of [0, 2p) values (the pairing levels' operands) against lazy values
            y = L[rng.randrange(len(L))]
            R.append([lsub(x, y)] if unary else [lsub(x, y), L[rng.randrange(len(L))]])
        # at the limb bound: |a_i| = 2^29 - 1 against the largest |b_j| the product bound allows, every sign pattern
        a_max = (1 << 29) - 1
        b_max = (1 << 29) - 1 if unary else mul_s_prod_max(p) // a_max
        pats = [lambda i: 1, lambda i: -1, lambda i: 1 if i & 1 else -1]
        for sa in pats:
            if unary:
                R.append([raw_limbs([sa(i) * a_max for i in range(NL)])])
                continue
            for sb in pats:
                R.append([raw_limbs([sa(i) * a_max for i in range(NL)]), raw_limbs([sb(i) * b_max for i in range(NL)])])
        if not unary:                   # |a_i| up to 2^30 - 1 (the stated 2^30 x 2^28 case, kept inside the product bound)
            a30 = (1 << 30) - 1
            b30 = mul_s_prod_max(p) // a30
            for sa in pats:
                for sb in pats:
                    R.append([raw_limbs([sa(i) * a30 for i in range(NL)]), raw_limbs([sb(i) * b30 for i in range(NL)])])
        for _ in range(n_random):
            if unary:
                R.append([raw_limbs([rng.randint(-a_max, a_max) for _ in range(NL)])] if rng.random() < 0.5 else [lsub(rl(), rl())])
            else:
                r = rng.random()
                if r < 0.4:
                    R.append([lsub(rl(), rl()), rl()])
                elif r < 0.7:
                    R.append([raw_limbs([rng.randint(-a_max, a_max) for _ in range(NL)]),
                              raw_limbs([rng.randint(-b_max, b_max) for _ in range(NL)])])
                else:
                    a = raw_limbs([s32(x) + s32(y) for x, y in zip(lsub(rl(), rl()), rl())])
                    R.append([a, rl()])
    elif op in (SUB_RAW, ADDSUB_RAW):   # limbs of |.| < 2^29 (stage outputs, differences): no int32 overflow in the result
        def rawop():
            r = rng.random()
            if r < 0.3:
                return rl()
            if r < 0.6:
                return lsub(rl(), rl())
            return raw_limbs([rng.randint(-(1 << 29) + 1, (1 << 29) - 1) for _ in range(NL)])
        for x in L:
            for y in L[::3]:
                R.append([x, y])
        m29 = (1 << 29) - 1
        for sa in (1, -1):
            for sb in (1, -1):
                R.append([raw_limbs([sa * m29] * NL), raw_limbs([sb * m29] * NL)])
        R += [[rawop(), rawop()] for _ in range(n_random)]
        if op == ADDSUB_RAW:
            recs[1] = [list(r) for r in R]
    elif op == NORM:                    # signed limbs, |limb| < 2^30, |value| < 5p
        vals = []
        for kk in range(-5, 5):         # within 2^-20 p of (k + 1/2) p: where the float quotient's floor decides
            c = (2 * kk + 1) * p // 2
            d = p >> 20
            vals += [c - d, c - 1, c, c + 1, c + d] + [c + rng.randint(-d, d) for _ in range(8)]
        vals += [-5 * p + 1, 5 * p - 1, 0, p, -p, 2 * p, -2 * p]
        vals += [rng.randint(-5 * p + 1, 5 * p - 1) for _ in range(n_random)]
        for v in vals:
            if not -5 * p < v < 5 * p:
                continue
            R.append([to_limbs(v)])
            for push in (True, False):
                s = scramble(v, norm_limb_bound(v, p), rng, push)
                if s is not None:
                    R.append([s])
    elif op == RAW_MAYBE_ZERO:          # d = a - b limb-wise, a, b in [0, 2p)
        Lp = [to_limbs(v) for v in E if v < p]
        for x in Lp:
            R += [[lsub(x, x)], [lsub(to_limbs(val_std(x) + p), x)], [lsub(x, to_limbs(val_std(x) + p))]]
        for x in L:
            for y in L[::2]:
                R.append([lsub(x, y)])
        for _ in range(n_random):
            x = rng.randrange(p)
            r = rng.random()
            y = x + p if r < 0.2 else (x - p if r < 0.4 and x >= p else rng.randrange(2 * p))
            R.append([lsub(to_limbs(x), to_limbs(y))] if rng.random() < 0.5 else [lsub(to_limbs(y), to_limbs(x))])
            R.append([lsub(rl(), rl())])
    elif op == FROM_WIRE:               # canonical wire words (24 x u32) in limbs 0..23 of operand 0
        ws = [v for v in E if v < p] + [rng.randrange(p) for _ in range(n_random)]
        R += [[[(w >> (32 * j)) & 0xFFFFFFFF for j in range(24)] + [0, 0, 0]] for w in ws]
    elif op == TO_WIRE:
        R += [[x] for x in L] + [[rl()] for _ in range(n_random)]
    elif op == NTT2:                    # stage-A inputs in [0, 1.51p) with limbs < 2^28, twiddles in [0, 2p)
        hi = (151 * p + 99) // 100
        X = [to_limbs(v) for v in edge_values(p, hi, rng) + [hi - 1]]
        w_max = to_limbs(2 * p - 1)     # the largest twiddle
        rx = lambda: to_limbs(rng.randrange(hi) if rng.random() < 0.5 else rng.randrange(p, hi))
        base = []
        for x in X:
            base.append([x, X[-1], X[0], X[-1], w_max, w_max])        # xl, xh against the largest xh and twiddle
            base.append([X[0], x, X[0], X[-1], w_max, w_max])
            base.append([x, x, X[-1], x, L[rng.randrange(len(L))], L[rng.randrange(len(L))]])
        base += [[rx(), rx(), rx(), rx(), rl(), rl()] for _ in range(n_random // 2)]
        # towards the stage-B extremes: the stage-B lo input at its largest (sel 0) or smallest (sel 1), and, out of a few hundred
        # candidates, the hi input whose product with the largest twiddle comes out largest (the Montgomery quotient m near R')
        top = hi - 1
        for first in (0, 1):
            ta = (lambda v: v) if first else (lambda v: mont(2 * p - 1, v, p))
            for sel in (0, 1):
                sgn = -1 if sel else 1
                cands = [(rng.randrange(hi) if rng.random() < 0.5 else rng.randrange(p, hi), rng.randrange(p, hi)) for _ in range(300)]
                x2, x3 = max(cands, key=lambda c: mont(2 * p - 1, c[0] + sgn * ta(c[1]), p))
                x0, x1 = (top, top) if sel == 0 else (0, top)
                base.append([to_limbs(x0), to_limbs(x1), to_limbs(x2), to_limbs(x3), w_max, w_max])
        return {k: base for k in range(12)}
    else:
        raise ValueError(op)
    return recs


def records_array(ops_list):
    a = np.zeros((len(ops_list), IN_WORDS), dtype=np.uint32)
    for r, ops in enumerate(ops_list):
        for j, x in enumerate(ops):
            a[r, NL * j:NL * j + len(x)] = np.array([int(w) & 0xFFFFFFFF for w in x], dtype=np.uint64).astype(np.uint32)
    return a


# ---- the contracts -------------------------------------------------------------------------------------------------------------
def _mont_exact(r_val, prod, p):
    """r = (prod + m p) / R' for some 0 <= m < R': the Montgomery product exactly, i.e. r in [prod / R', prod / R' + p)"""
    d = r_val * RB - prod
    return d >= 0 and d < p * RB and d % p == 0


def check(mod, op, k, ops, out):
    """None if out (OUT_WORDS words) satisfies op's contract on operands ops, else a description"""
    p = MODS[mod]
    r0, r1, flag = [int(x) for x in out[:NL]], [int(x) for x in out[NL:2 * NL]], int(out[2 * NL])
    x = [[int(w) for w in o] for o in ops]
    xs = [val_std(o) for o in x]
    xr = [val_raw(o) for o in x]
    v0 = val_std(r0)
    rinv = pow(RB, -1, p)

    def lazy_out(v=v0, lim=r0):
        return normalised(lim) and 0 <= v < 2 * p

    if op in (MUL, SQR, MUL2):
        prod = xs[0] * xs[1] if op == MUL else (xs[0] * xs[0] if op == SQR else xs[0] * xs[1] + xs[2] * xs[3])
        if not normalised(r0):
            return "result limbs not in [0, 2^28)"
        if not _mont_exact(v0, prod, p):
            return "not the Montgomery product (residue, or outside [ab / R', ab / R' + p))"
        if v0 >= 2 * p:
            return "result >= 2p"
    elif op == MUL3:
        prod = xs[0] * xs[1] + xs[2] * xs[3] + xs[4] * xs[5]
        if not lazy_out():
            return "result not in [0, 2p) with normalised limbs"
        if (v0 - prod * rinv) % p:
            return "wrong residue"
    elif op == REDUCE2P:
        want = xs[0] - 2 * p if xs[0] >= 2 * p else xs[0]
        if r0 != to_limbs(want):
            return "not s mod 2p"
    elif op in (ADD, SUB, NEG):
        s = xs[0] + xs[1] if op == ADD else ((xs[0] - xs[1] + 2 * p) if op == SUB else 2 * p - xs[0])
        want = s - 2 * p if s >= 2 * p else s
        if r0 != to_limbs(want):
            return "not the reduced sum / difference in [0, 2p)"
    elif op == HALF:
        a = xs[0]
        if not normalised(r0):
            return "result limbs not in [0, 2^28)"
        if (2 * v0 - a) % p or v0 > (a + p) // 2:
            return "not a / 2, or above (a + p) / 2"
    elif op == MUL_SMALL:
        if not lazy_out():
            return "result not in [0, 2p) with normalised limbs"
        if (v0 - k * xs[0]) % p:
            return "wrong residue"
    elif op in (MUL_S, MUL_S_IP, SQR_S, SQR_S_KEEP):
        prod = xr[0] * xr[1] if op in (MUL_S, MUL_S_IP) else xr[0] * xr[0]
        if not normalised(r0[:NL - 1]):
            return "limbs 0..25 not in [0, 2^28)"
        if not _mont_exact(v0, prod, p):
            return "not the Montgomery product (residue, or outside [ab / R', ab / R' + p))"
        if op in (MUL_S_IP, SQR_S_KEEP) and r1 != x[0]:
            return "the kept operand changed"
    elif op in (SUB_RAW, ADDSUB_RAW):
        sign = -1 if (op == SUB_RAW or (k & 1)) else 1
        want = [s32(a) + sign * s32(b) for a, b in zip(x[0], x[1])]
        if [s32(w) for w in r0] != want:
            return "limb-wise result wrong"
        if val_raw(r0) != xr[0] + sign * xr[1]:
            return "value wrong"
    elif op == NORM:
        if not normalised(r0):
            return "result limbs not in [0, 2^28)"
        if (v0 - xr[0]) % p:
            return "wrong residue"
        if not (49 * p <= 100 * v0 < 151 * p):
            return f"result {v0 / p:.8f} p outside [0.49p, 1.51p)"
    elif op == RAW_MAYBE_ZERO:
        t = x[0][0] & MASK
        want = t in (0, MODS[mod] & MASK, (-MODS[mod]) & MASK)
        if flag != int(want):
            return "not the low-limb predicate"
        if xr[0] in (-p, 0, p) and not flag:
            return "a zero difference not flagged"
    elif op == IS_ZERO:
        if flag != int(xs[0] % p == 0):
            return "wrong zero test"
    elif op == CANON:
        if r0 != to_limbs(xs[0] % p):
            return "not a mod p"
    elif op == INV:
        if not lazy_out():
            return "result not in [0, 2p) with normalised limbs"
        a = xs[0] % p
        want = 0 if a == 0 else (pow(2, 1512, p) * pow(a, -1, p)) % p
        if v0 % p != want:
            return "not 2^1512 / x"
    elif op == FROM_WIRE:
        w = sum(x[0][j] << (32 * j) for j in range(24))
        if not lazy_out():
            return "result not in [0, 2p) with normalised limbs"
        if (v0 - w * pow(2, -12, p)) % p:
            return "not w 2^-12"
    elif op == TO_WIRE:
        w = sum(r0[j] << (32 * j) for j in range(24))
        if w != (xs[0] << 12) % p or any(r0[24:]):
            return "not the canonical a 2^12"
    elif op == NTT2:
        t = lambda w, v: v * w * rinv
        sel, first, stage = k & 1, (k >> 1) & 1, k >> 2
        sgn = -1 if sel else 1
        ta = (lambda v: v) if first else (lambda v: t(xs[4], v))               # the first stage of a transform: t = x_hi
        a = [xs[0] + sgn * ta(xs[1]), xs[2] + sgn * ta(xs[3])]                  # stage-A outputs feeding stage B (mod p)
        b = [a[0] + t(xs[5], a[1]), a[0] - t(xs[5], a[1])]
        want = a if stage == 0 else b
        v = [val_raw(r0), val_raw(r1)]
        for j in range(2):
            if (v[j] - want[j]) % p:
                return f"stage {stage}: output {j} wrong residue"
        # the ranges of ntt_kernels.hip.h (k_ntt_group), in hundredths of p: (after a product stage, after the first stage)
        if stage == 0:
            lo, hi = (-151, 302) if first else (-134, 285)
            if not all(lo * p < 100 * vj < hi * p for vj in v) or max(max_abs_limb(r0), max_abs_limb(r1)) >= (1 << 29):
                return f"stage-A output {[vj / p for vj in v]} p outside ({lo / 100}p, {hi / 100}p) or a limb >= 2^29"
        elif stage == 1:
            lo, hi = (-318, 469) if first else (-297, 448)
            if not all(lo * p < 100 * vj < hi * p for vj in v) or max(max_abs_limb(r0), max_abs_limb(r1)) >= 3 << LB:
                return f"stage-B output {[vj / p for vj in v]} p outside ({lo / 100}p, {hi / 100}p) or a limb >= 3 2^28"
        else:
            for lim, vj in ((r0, v[0]), (r1, v[1])):
                if not normalised(lim) or not (49 * p <= 100 * vj < 151 * p):
                    return f"normalised output {vj / p:.8f} p outside [0.49p, 1.51p)"
    return None


def run_op(hook, mod, op, seed=1, n_random=1500, twin=None):
    """Run every case of (mod, op) through hook(mod, op, records, k) -> (n, OUT_WORDS); assert each result's contract.  twin: a
    second hook whose output must be bit-identical wherever fp_norm is not involved.  Returns the number of records checked."""
    rng = random.Random(seed * 1000 + 10 * op + mod)
    total, bad = 0, []
    for k, ops_list in cases(mod, op, rng, n_random).items():
        if not ops_list:
            continue
        rec = records_array(ops_list)
        out = hook(mod, op, rec, k)
        assert out.shape == (len(ops_list), OUT_WORDS)
        if twin is not None and not involves_norm(op, k):
            ref = twin(mod, op, rec, k)
            diff = np.nonzero(np.any(out != ref, axis=1))[0]
            for i in diff[:3]:
                bad.append(f"k={k} record {i}: differs from the host twin")
        for i, ops in enumerate(ops_list):
            msg = check(mod, op, k, ops, out[i])
            if msg:
                bad.append(f"k={k} record {i}: {msg}; operands {[hex(val_raw(o)) for o in ops]}")
        total += len(ops_list)
    assert not bad, f"{OP_NAMES[op]} mod {mod}: {len(bad)} failures of {total}:\n" + "\n".join(bad[:10])
    return total


def build_host_twin(out_dir):
    so = os.path.join(str(out_dir), "libfield_raw_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tools", "host_tests", "field_raw_host.cpp")],
                   check=True, timeout=600)
    L = C.CDLL(so)
    u32p = C.POINTER(C.c_uint32)
    L.mnt753_test_field_raw.restype = C.c_int
    L.mnt753_test_field_raw.argtypes = [C.c_int, C.c_int, u32p, C.c_size_t, C.c_uint32, u32p]

    def hook(mod, op, records, k=0):
        rec = np.ascontiguousarray(records, dtype=np.uint32)
        out = np.zeros((rec.shape[0], OUT_WORDS), dtype=np.uint32)
        assert L.mnt753_test_field_raw(mod, op, rec.ctypes.data_as(u32p), rec.shape[0], k, out.ctypes.data_as(u32p)) == 0
        return out
    return hook


# ---- extension fields with raw components --------------------------------------------------------------------------------------
def ext_case_components(mod, rng, n):
    """n elements' components, each from the edge set of [0, 2p) or random in [0, 2p)"""
    p = MODS[mod]
    E = edge_values(p, 2 * p, rng)
    return [E[rng.randrange(len(E))] if rng.random() < 0.5 else rand_lazy(p, rng) for _ in range(n)]
