"""Compressed points of MNT4753 / MNT6753 in Python integers (TEST INFRASTRUCTURE): the packed form of include/mnt753_hip.h
("compressed points"), its decompression rules and libff's stream records, on top of tests/designed_points.py (f_sqrt, curve_rhs) and
tools/pyref.py.  Nothing here uses the project's arithmetic.

Packed form of n points of (curve, group): x [n, Wx] uint64 wire words (Wx = 12 deg), flags [n] uint8 -- bit 0 the parity of y as an
integer in [0, q) (G2: of y.c0), bit 1 the identity.  decompress, per point, the first rule that applies: a flag bit 2-7 or a
component of x >= q -> BAD_NONCANONICAL; the identity flag -> zero words, good; x^3 + a x + b not a square, or zero -> BAD_OFF_CURVE;
else the root whose parity is bit 0 (y.c0 = 0: the root whose first non-zero higher component is even).  A bad point is zero words.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pyref  # noqa: E402
import designed_points as DP  # noqa: E402

CURVES = DP.CURVES
BAD_NONE, BAD_NONCANONICAL, BAD_OFF_CURVE = 0, 1, 2
FLAG_ODD, FLAG_IDENTITY = 1, 2
GROUPS = [(0, 1), (0, 2), (1, 1), (1, 2)]


def degree(curve, group):
    return DP.degree(curve, group)


def x_words(curve, group):
    return 12 * degree(curve, group)


def record_bytes(curve, group):
    return 8 * x_words(curve, group) + 2


def parity(y):
    """libff's Y.as_bigint().data[0] & 1 (G2: of Y.c0)"""
    return (y if isinstance(y, int) else y[0]) & 1


def sign_key(y):
    """the index of the component that decides the sign: the first non-zero one (c0 unless it is zero)"""
    if isinstance(y, int):
        return 0
    return next((k for k, v in enumerate(y) if v), 0)


def pick_root(curve, y, odd):
    """of y and -y the one the flag names"""
    cv = CURVES[curve]
    k = sign_key(y)
    comp = y if isinstance(y, int) else y[k]
    want = odd if k == 0 else 0
    return y if (comp & 1) == want else cv.f_neg(y)


def compress_point(curve, group, pt):
    """a pyref point (None: the identity) -> (x words, flag)"""
    cv = CURVES[curve]
    if pt is None:
        return [0] * x_words(curve, group), FLAG_IDENTITY
    return cv.coord_to_words(pt[0]), parity(pt[1])


def compress(curve, group, words):
    """affine wire words [n, 2 Wx] -> (x [n, Wx], flags [n]); validates nothing"""
    w = np.asarray(words, dtype=np.uint64).reshape(-1, 2 * x_words(curve, group))
    xs, fl = [], []
    for row in w:
        x, f = compress_point(curve, group, DP.from_words(curve, group, row))
        xs.append(x)
        fl.append(f)
    return np.array(xs, dtype=np.uint64).reshape(len(fl), x_words(curve, group)), np.array(fl, dtype=np.uint8)


def decompress_point(curve, group, xw, flag):
    """-> (pyref point or None, reason)"""
    cv, deg = CURVES[curve], degree(curve, group)
    ints = [pyref.Curve.words_to_int(xw[12 * k:12 * k + 12]) for k in range(deg)]
    if flag & 0xFC or any(v >= cv.q for v in ints):
        return None, BAD_NONCANONICAL
    if flag & FLAG_IDENTITY:
        return None, BAD_NONE
    x = cv.coord_from_words([int(v) for v in xw], deg)
    rhs = DP.curve_rhs(curve, group, x)
    y = DP.f_sqrt(curve, rhs)
    if y is None or cv.f_is_zero(y):
        return None, BAD_OFF_CURVE
    return (x, pick_root(curve, y, flag & 1)), BAD_NONE


def decompress(curve, group, x, flags):
    """-> (affine wire words [n, 2 Wx], (n_bad, first_bad, reason of first_bad))"""
    wx = x_words(curve, group)
    xs = np.asarray(x, dtype=np.uint64).reshape(-1, wx)
    fl = np.asarray(flags, dtype=np.uint8).reshape(-1)
    out = np.zeros((len(fl), 2 * wx), dtype=np.uint64)
    n_bad, first, reason = 0, 0, BAD_NONE
    for i, (row, f) in enumerate(zip(xs, fl)):
        pt, why = decompress_point(curve, group, [int(v) for v in row], int(f))
        if why != BAD_NONE:
            if n_bad == 0:
                first, reason = i, why
            n_bad += 1
        elif pt is not None:
            out[i] = DP.to_words(curve, group, pt)
    return out, (n_bad, first, reason)


# ---- libff's stream records (BINARY_OUTPUT + MONTGOMERY_OUTPUT, empty OUTPUT_SEPARATOR) ------------------------------------------------
def to_stream(curve, group, x, flags):
    wx = x_words(curve, group)
    xs = np.ascontiguousarray(x, dtype="<u8").reshape(-1, wx)
    out = bytearray()
    for row, f in zip(xs, np.asarray(flags, dtype=np.uint8).reshape(-1)):
        if f & 0xFC:
            raise ValueError("a flag byte has a bit above the identity flag set")
        if f & FLAG_IDENTITY:
            out += b"1" + bytes(8 * wx) + b"1"         # zero() after to_affine_coordinates(): X = 0, Y = 1
        else:
            out += b"0" + row.tobytes() + (b"1" if f & 1 else b"0")
    return bytes(out)


def from_stream(curve, group, data, n=None):
    wx, rec = x_words(curve, group), record_bytes(curve, group)
    n = len(data) // rec if n is None else n
    if len(data) < n * rec:
        raise ValueError("the buffer is shorter than n records")
    xs = np.zeros((n, wx), dtype=np.uint64)
    fl = np.zeros(n, dtype=np.uint8)
    for i in range(n):
        r = data[i * rec:(i + 1) * rec]
        zero, par = r[0:1], r[-1:]
        if zero not in (b"0", b"1") or par not in (b"0", b"1"):
            raise ValueError("a flag byte is neither '0' nor '1'")
        if zero == b"1":
            fl[i] = FLAG_IDENTITY
        else:
            xs[i] = np.frombuffer(r[1:-1], dtype="<u8")
            fl[i] = 1 if par == b"1" else 0
    return xs, fl


# ---- proofs ---------------------------------------------------------------------------------------------------------------------------
def proof_parts(curve):
    """[(group, first word, words)] of A | B | C in an affine proof"""
    w2 = 24 * CURVES[curve].deg
    return [(1, 0, 24), (2, 24, w2), (1, 24 + w2, 24)]


def compress_proofs(curve, proofs):
    """affine proofs [n, 48 + w2] -> (x [n, 24 + w2 / 2], flags [n, 3])"""
    p = np.asarray(proofs, dtype=np.uint64).reshape(-1, 48 + 24 * CURVES[curve].deg)
    xs, fl = [], []
    for group, at, words in proof_parts(curve):
        x, f = compress(curve, group, p[:, at:at + words])
        xs.append(x)
        fl.append(f)
    return np.concatenate(xs, axis=1), np.stack(fl, axis=1)


def proof_to_stream(curve, x, flags):
    """one compressed proof -> its 390 / 486 stream bytes: the records of A, B, C back to back"""
    x = np.asarray(x, dtype=np.uint64).reshape(-1)
    out, at = b"", 0
    for k, (group, _, _) in enumerate(proof_parts(curve)):
        wx = x_words(curve, group)
        out += to_stream(curve, group, x[at:at + wx], [int(np.asarray(flags).reshape(-1)[k])])
        at += wx
    return out


def proof_from_stream(curve, data):
    xs, fl, at = [], [], 0
    for group, _, _ in proof_parts(curve):
        rec = record_bytes(curve, group)
        x, f = from_stream(curve, group, data[at:at + rec], 1)
        xs.append(x.reshape(-1))
        fl.append(int(f[0]))
        at += rec
    if at != len(data):
        raise ValueError("a compressed proof is three records")
    return np.concatenate(xs), np.array(fl, dtype=np.uint8)


# ---- designed inputs --------------------------------------------------------------------------------------------------------------------
NON_LIFTABLE_X = {(0, 1): 3, (0, 2): (1, 1), (1, 1): 1, (1, 2): (2, 1, 0)}     # small x whose rhs is not a square


def non_liftable_words(curve, group):
    cv = CURVES[curve]
    x = NON_LIFTABLE_X[(curve, group)]
    assert DP.lift(curve, group, x) is None and not cv.f_is_zero(DP.curve_rhs(curve, group, x))
    return np.array(cv.coord_to_words(x), dtype=np.uint64)


def two_adic(curve, deg):
    """(s, t, c): |F| - 1 = 2^s t, c = z^t of order 2^s for the non-residue z of designed_points._two_adic"""
    return DP._two_adic(curve, deg)


def sqrt_designed_set(curve, deg, seed=7):
    """[(name, element, is a square)] for the square-root hook: with c = z^t and u random, c^(2^(s - k)) u^(2^s) for EVERY k = 0 .. s - 1
    (a^t has order exactly 2^k: Tonelli-Shanks depth k); 0, 1, q - 1, the all-(q - 1) element; the non-squares z^t, z^t u^2 and, in
    the extensions, one with zero c0.  Ordered so that neighbours differ in depth and squares mix with non-squares."""
    cv = CURVES[curve]
    q = cv.q
    s, t, c = two_adic(curve, deg)
    rng = pyref.splitmix64(seed)

    def rand():
        v = [pyref.rand_below(rng, q - 1) + 1 for _ in range(deg)]
        return v[0] if deg == 1 else tuple(v)

    def embed(v):
        return v % q if deg == 1 else tuple([v % q] + [0] * (deg - 1))
    euler = lambda a: cv.f_is_zero(a) or DP.f_pow(cv, a, (q ** deg - 1) // 2) == cv.f_one(a)
    depth = []
    for k in range(s):
        u = DP.f_pow(cv, rand(), 1 << s)
        zk = DP.f_pow(cv, c, 1 << (s - k))
        depth.append((f"depth{k}", cv.f_mul(zk, u), True))
    allm = q - 1 if deg == 1 else tuple([q - 1] * deg)
    u2 = cv.f_mul(rand(), rand())
    u2 = cv.f_mul(u2, u2)
    others = [("0", embed(0), True), ("1", embed(1), True), ("q-1", embed(q - 1), euler(embed(q - 1))), ("all(q-1)", allm, euler(allm)),
              ("z^t", c, False), ("z^t u^2", cv.f_mul(c, u2), False)]
    if deg > 1:
        k = 2
        while True:                                 # the first non-square (0, k[, 1])
            a = tuple([0, k] + [1] * (deg - 2))
            if not euler(a):
                break
            k += 1
        others.append(("zero c0", a, False))
    # interleave: shallow and deep depths alternate, a special element after every third
    order = []
    lo, hi = 0, len(depth) - 1
    while lo <= hi:
        order.append(depth[lo]); lo += 1
        if lo <= hi:
            order.append(depth[hi]); hi -= 1
    out, oi = [], 0
    for i, e in enumerate(order):
        out.append(e)
        if i % 3 == 2 and oi < len(others):
            out.append(others[oi]); oi += 1
    out += others[oi:]
    return out
