"""Big-integer model of the input checks (csrc/mnt753_validate.hip), on top of tools/pyref.py: what tests/test_validate_gpu.py
compares the device with, and what tests/test_validate_cpu.py pins to the reference's own data.  Per point, in this order: a
coordinate component >= q -> BAD_NONCANONICAL; all words of y zero -> the identity, well formed (serialization.hpp:84-111); the curve
equation of pyref.Curve.on_curve (libff's is_well_formed) -> BAD_OFF_CURVE."""
import numpy as np

import pyref

OK, NONCANONICAL, OFF_CURVE, UNSATISFIED = 0, 1, 2, 3
R = 1 << 768
CURVES = {0: pyref.Curve(0), 1: pyref.Curve(1)}
_RINV = {}


def rinv(mod):
    if mod not in _RINV:
        _RINV[mod] = pow(R, -1, mod)
    return _RINV[mod]


def ints(words):
    """u64 array (..., 12 k) -> list of k Python integers, one per 12 words"""
    raw = np.ascontiguousarray(words, dtype=np.uint64).tobytes()
    return [int.from_bytes(raw[i:i + 96], "little") for i in range(0, len(raw), 96)]


def to_words(values):
    """list of integers below 2^768 -> u64 array (n, 12)"""
    return np.frombuffer(b"".join(int(v).to_bytes(96, "little") for v in values), dtype=np.uint64).reshape(len(values), 12).copy()


def degree(curve, group):
    return 1 if group == 1 else CURVES[curve].deg


def point_verdict(curve, group, words):
    cv, deg = CURVES[curve], degree(curve, group)
    comps = ints(words)
    assert len(comps) == 2 * deg
    if any(c >= cv.q for c in comps):
        return NONCANONICAL
    if all(c == 0 for c in comps[deg:]):
        return OK
    vals = [c * rinv(cv.q) % cv.q for c in comps]
    x, y = (vals[0], vals[1]) if deg == 1 else (tuple(vals[:deg]), tuple(vals[deg:]))
    return OK if cv.on_curve((x, y), group) else OFF_CURVE


def point_verdicts(curve, group, pts):
    return [point_verdict(curve, group, p) for p in pts]


def scalar_verdicts(curve, scalars):
    r = CURVES[curve].r
    return [NONCANONICAL if v >= r else OK for v in ints(scalars)]


def product_verdicts(curve, a, b, c):
    """rows a[i] b[i] == c[i] on wire words (x R mod r): a row with a word >= r is NONCANONICAL, a failing product UNSATISFIED"""
    r = CURVES[curve].r
    out = []
    for x, y, z in zip(ints(a), ints(b), ints(c)):
        if x >= r or y >= r or z >= r:
            out.append(NONCANONICAL)
        else:
            out.append(OK if (x * y - z * R) % r == 0 else UNSATISFIED)     # (a R)(b R) = (c R) R
    return out


def report(verdicts):
    """-> (n_bad, first_bad, reason of first_bad) as mnt753_check_report holds them"""
    bad = [i for i, v in enumerate(verdicts) if v != OK]
    return (len(bad), bad[0], verdicts[bad[0]]) if bad else (0, 0, OK)


def params_sets(curve, path):
    """-> d, m, {name: (group, byte offset, count, u64 array (count, words))} of a parameter file"""
    raw = np.fromfile(path, dtype=np.uint64)
    d, m = int(raw[0]), int(raw[1])
    g1w, g2w = 24, 24 * CURVES[curve].deg
    sets, pos = {}, 2
    for name, group, words, n in (("A", 1, g1w, m + 1), ("B1", 1, g1w, m + 1), ("B2", 2, g2w, m + 1), ("L", 1, g1w, m - 1), ("H", 1, g1w, d)):
        sets[name] = (group, 8 * pos, n, raw[pos:pos + words * n].reshape(n, words))
        pos += words * n
    assert pos == raw.size
    return d, m, sets


def input_vectors(path, d, m):
    """-> {name: u64 array (n, 12)} of an input file: w[m + 1], ca / cb / cc [d + 1], r"""
    raw = np.fromfile(path, dtype=np.uint64).reshape(-1, 12)
    assert raw.shape[0] == m + 1 + 3 * (d + 1) + 1
    n = d + 1
    return {"w": raw[:m + 1], "ca": raw[m + 1:m + 1 + n], "cb": raw[m + 1 + n:m + 1 + 2 * n], "cc": raw[m + 1 + 2 * n:m + 1 + 3 * n], "r": raw[-1:]}
