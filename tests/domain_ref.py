"""Python-integer checker for evaluation domains beyond powers of two (TEST INFRASTRUCTURE).

Independent of libfqfft's algorithms where it matters: a transform is checked against its DEFINITION -- FFT(a)[idx] is the value of the
polynomial sum a_k x^k at the domain's idx-th element (Horner), an inverse transform is pinned by applying that FFT to its result
(the map is a bijection), the coset variants evaluate at g * element, and divide_by_Z_on_coset divides by the vanishing polynomial at
g * element(idx).  Field results are canonical, so equality with libfqfft is word for word.

`select` models the walk of libfqfft's get_evaluation_domain (candidates 1-7, each with its constructor's acceptance test), including
the mixed-radix acceptance of MNT6753's Fr (small subgroup 5^2).

The `fast_*` functions are the O(m log m) composition -- the O(m) passes in Python around the oracle's radix-2 FFT -- for sizes where
O(m^2) integers are too slow; tests/test_domains_cpu.py pins them to the definition at small sizes.

Elements are Python integers in [0, r) unless a function says "wire" (numpy uint64 [m, 12], Montgomery R = 2^768, the ABI's format).
"""
import operator
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import mnt753_params as P  # noqa: E402

R = 1 << 768
G = P.MULTIPLICATIVE_GENERATOR
MODULUS = {0: P.MOD_A, 1: P.MOD_B}                     # Fr of MNT4753 / MNT6753
TWO_ADICITY = {0: P.A_TWO_ADICITY, 1: P.B_TWO_ADICITY}
ROOT = {0: P.A_ROOT_OF_UNITY, 1: P.B_ROOT_OF_UNITY}
SMALL_SUBGROUP = {0: None, 1: (P.B_SMALL_SUBGROUP_BASE, P.B_SMALL_SUBGROUP_POWER, P.B_FULL_ROOT_OF_UNITY)}

BASIC, EXTENDED, STEP = "basic", "extended", "step"
MIXED, MIXED_EXTENDED, SEQUENCE, NONE = "mixed", "mixed-extended", "sequence", "none"     # what the library refuses
KIND_CODE = {BASIC: 0, EXTENDED: 1, STEP: 2}          # MNT753_DOMAIN_*


def clog2(n):
    """libff::log2: the ceiling"""
    r = 0
    while (1 << r) < n:
        r += 1
    return r


def is_pow2(n):
    return n > 0 and n & (n - 1) == 0


def _adicity(k, n):
    r = 0
    while n > 1 and n % k == 0:
        n //= k
        r += 1
    return r


def root_of_unity(curve, n):
    """libff get_root_of_unity(n): a primitive n-th root, or None where it reports an error"""
    r, s = MODULUS[curve], TWO_ADICITY[curve]
    if n == 0:
        return None
    if SMALL_SUBGROUP[curve]:
        q, qpow, full = SMALL_SUBGROUP[curve]
        qa, ta = _adicity(q, n), _adicity(2, n)
        if n != (1 << ta) * q ** qa or ta > s or qa > qpow:
            return None
        w = full
        for _ in range(qpow - qa):
            w = pow(w, q, r)
        for _ in range(s - ta):
            w = w * w % r
        return w
    ln = clog2(n)
    if n != 1 << ln or ln > s:
        return None
    w = ROOT[curve]
    for _ in range(s - ln):
        w = w * w % r
    return w


def basic_accepts(curve, m):
    if m <= 1:
        return False
    if SMALL_SUBGROUP[curve]:
        q = SMALL_SUBGROUP[curve][0]
        if m != q ** _adicity(q, m) * (1 << _adicity(2, m)):
            return False
        return root_of_unity(curve, m) is not None
    return clog2(m) <= TWO_ADICITY[curve] and root_of_unity(curve, m) is not None


def extended_accepts(curve, m):
    return m > 1 and clog2(m) == TWO_ADICITY[curve] + 1 and root_of_unity(curve, m // 2) is not None


def step_split(m):
    big = 1 << (clog2(m) - 1)
    return big, m - big


def step_accepts(curve, m):
    if m <= 1:
        return False
    big, small = step_split(m)
    if small != 1 << clog2(small):
        return False
    return root_of_unity(curve, 1 << clog2(m)) is not None and root_of_unity(curve, small) is not None


def best_mixed_domain_size(curve, min_size):
    q, qpow, _ = SMALL_SUBGROUP[curve]
    best = None
    for b in range(qpow + 1):
        r, a = q ** b, 0
        while r < min_size:
            r *= 2
            a += 1
        if a <= TWO_ADICITY[curve] and (best is None or r < best):
            best = r
    return best


def select(curve, min_size):
    """-> (kind, m): the domain the reference builds for min_size.  BASIC / EXTENDED / STEP are plain radix-2 domains (the library
    builds them); MIXED (a basic domain with a radix-5 part), MIXED_EXTENDED, SEQUENCE (past candidate 7) and NONE (0, 1) are refused."""
    if min_size <= 1:
        return NONE, 0
    big = 1 << (clog2(min_size) - 1)
    small = min_size - big
    for m in (min_size, big + (1 << clog2(small))):      # candidates 1-3, then 4-6
        if basic_accepts(curve, m):
            return (BASIC if is_pow2(m) else MIXED), m
        if extended_accepts(curve, m):
            return (EXTENDED if m % 2 == 0 and is_pow2(m // 2) else MIXED_EXTENDED), m
        if step_accepts(curve, m):
            return STEP, m
    if SMALL_SUBGROUP[curve]:                            # candidate 7
        s = best_mixed_domain_size(curve, min_size)
        if s is not None and basic_accepts(curve, s):
            return (BASIC if is_pow2(s) else MIXED), s
    return SEQUENCE, min_size


# ---- the domains by definition ------------------------------------------------------------------------------------------------------
def _parts(curve, kind, m):
    """(size of the first part, root of the first part, offset of the second part, root of the second part)"""
    r = MODULUS[curve]
    if kind == BASIC:
        return m, root_of_unity(curve, m), 0, 1
    if kind == EXTENDED:
        return m // 2, root_of_unity(curve, m // 2), G * G % r, root_of_unity(curve, m // 2)     # shift = g^2 (libff coset_shift)
    big, small = step_split(m)
    omega = root_of_unity(curve, 1 << clog2(m))
    return big, omega * omega % r, omega, root_of_unity(curve, small)


def element(curve, kind, m, idx):
    """get_domain_element(idx)"""
    r = MODULUS[curve]
    n0, w0, off, w1 = _parts(curve, kind, m)
    return pow(w0, idx, r) if idx < n0 else off * pow(w1, idx - n0, r) % r


def elements(curve, kind, m):
    r = MODULUS[curve]
    n0, w0, off, w1 = _parts(curve, kind, m)
    out, x = [], 1
    for _ in range(n0):
        out.append(x)
        x = x * w0 % r
    x = off
    for _ in range(m - n0):
        out.append(x)
        x = x * w1 % r
    return out


def _vanishing_form(curve, kind, m):
    """(A, B, C): Z(t) = (t^A - 1) (t^B - C)"""
    r = MODULUS[curve]
    if kind == BASIC:
        return m, 0, 0
    if kind == EXTENDED:
        return m // 2, m // 2, pow(G * G, m // 2, r)
    big, small = step_split(m)
    return big, small, pow(root_of_unity(curve, 1 << clog2(m)), small, r)


def vanishing(curve, kind, m, t):
    """compute_vanishing_polynomial(t): the monic polynomial of degree m that is zero on the domain"""
    r = MODULUS[curve]
    A, B, C = _vanishing_form(curve, kind, m)
    return (pow(t, A, r) - 1) * (pow(t, B, r) - C) % r


def _horner(coeffs, x, r):
    """sum coeffs[k] x^k mod r: Horner's rule in x^1024 over blocks whose inner sums sum a_k x^k are reduced once"""
    block = min(1024, len(coeffs))
    pw = _powers(x, block, r)
    xb = pw[-1] * x % r
    acc = 0
    for j in reversed(range(0, len(coeffs), block)):
        acc = (acc * xb + sum(map(operator.mul, coeffs[j:j + block], pw))) % r
    return acc


_POOL_POLYS = None


def _pool_init(packed, r):
    global _POOL_POLYS
    _POOL_POLYS = ([mont_ints(np.frombuffer(b, dtype="<u8")) for b in packed], r)


def _pool_eval(task):
    polys, r = _POOL_POLYS
    return _horner(polys[task[0]], task[1], r)


def eval_many(polys, tasks, r, workers=8):
    """[polys[k](x) mod r for (k, x) in tasks].  Above 2^24 coefficient products the tasks are spread over freshly started Python
    processes (pure integer work: they import this module only and never touch a GPU)."""
    if sum(len(polys[k]) for k, _ in tasks) < (1 << 24) or workers <= 1:
        return [_horner(polys[k], x, r) for k, x in tasks]
    import multiprocessing as mp
    packed = [ints_to_words(p).tobytes() for p in polys]
    with mp.get_context("spawn").Pool(min(workers, os.cpu_count() or 1), _pool_init, (packed, r)) as pool:
        return pool.map(_pool_eval, tasks, chunksize=4)


def fft_at(curve, kind, m, a, idx, coset=False):
    """FFT(a)[idx] (cosetFFT with coset=True) by definition"""
    r = MODULUS[curve]
    x = element(curve, kind, m, idx)
    return _horner(a, G * x % r if coset else x, r)


def fft_def(curve, kind, m, a, coset=False):
    r = MODULUS[curve]
    return [_horner(a, G * x % r if coset else x, r) for x in elements(curve, kind, m)]


def is_ifft_of(curve, kind, m, coeffs, values, coset=False):
    """coeffs == iFFT(values) (icosetFFT with coset=True): FFT of the result gives the input back"""
    return fft_def(curve, kind, m, coeffs, coset) == list(values)


def divide_by_z_on_coset_def(curve, kind, m, p):
    r = MODULUS[curve]
    return [v * pow(vanishing(curve, kind, m, G * x % r), -1, r) % r for v, x in zip(p, elements(curve, kind, m))]


# ---- wire format ------------------------------------------------------------------------------------------------------------------------
def from_wire(curve, words):
    """numpy uint64 [n, 12] -> integers in [0, r)"""
    r = MODULUS[curve]
    rinv = pow(R, -1, r)
    return [v * rinv % r for v in mont_ints(words)]


def to_wire(curve, ints):
    r = MODULUS[curve]
    return ints_to_words([v * R % r for v in ints])


def mont_ints(words):
    """the raw Montgomery integers x R mod r of a wire array (the transforms are linear: they act on these as they act on x)"""
    raw = np.ascontiguousarray(words, dtype="<u8").reshape(-1, 12).tobytes()
    return [int.from_bytes(raw[o:o + 96], "little") for o in range(0, len(raw), 96)]


def ints_to_words(ints):
    return np.frombuffer(b"".join(v.to_bytes(96, "little") for v in ints), dtype="<u8").reshape(-1, 12).astype(np.uint64)


# ---- the fast composition: O(m) passes here, radix-2 transforms in the oracle -----------------------------------------------------------
def _radix2(curve, inverse, ints):
    """basic radix-2 FFT / iFFT (with its 1/n) of a power-of-two vector of integers, through oracle/liboracle.so"""
    if len(ints) == 1:
        return list(ints)
    import oracle_lib as O
    return mont_ints(O.fft(curve, 1 if inverse else 0, ints_to_words(ints).reshape(-1)))


def _powers(x, n, r, scale=1):
    out, v = [], scale % r
    for _ in range(n):
        out.append(v)
        v = v * x % r
    return out


def fast_fft(curve, kind, m, a, coset=False):
    """FFT / cosetFFT on integers (plain or Montgomery alike: the map is linear)"""
    r = MODULUS[curve]
    if coset:
        a = [v * gk % r for v, gk in zip(a, _powers(G, m, r))]
    if kind == BASIC:
        return _radix2(curve, False, a)
    if kind == EXTENDED:
        s = m // 2
        shift = G * G % r
        S = pow(shift, s, r)
        a0 = [(a[i] + a[s + i]) % r for i in range(s)]
        a1 = [sh * (a[i] + S * a[s + i]) % r for i, sh in enumerate(_powers(shift, s, r))]
        return _radix2(curve, False, a0) + _radix2(curve, False, a1)
    big, small = step_split(m)
    omega = root_of_unity(curve, 1 << clog2(m))
    c = [(a[i] + a[i + big]) % r if i < small else a[i] for i in range(big)]
    d = [w * ((a[i] - a[i + big]) if i < small else a[i]) % r for i, w in enumerate(_powers(omega, big, r))]
    e = [sum(d[i::small]) % r for i in range(small)]
    return _radix2(curve, False, c) + _radix2(curve, False, e)


def fast_ifft(curve, kind, m, v, coset=False):
    r = MODULUS[curve]
    if kind == BASIC:
        a = _radix2(curve, True, v)
    elif kind == EXTENDED:
        s = m // 2
        shift = G * G % r
        S = pow(shift, s, r)
        a0, a1 = _radix2(curve, True, v[:s]), _radix2(curve, True, v[s:])      # each with its 1/s
        k = pow(1 - S, -1, r)
        t = [x * si % r for x, si in zip(a1, _powers(pow(shift, -1, r), s, r))]
        a = [k * (t[i] - S * a0[i]) % r for i in range(s)] + [k * (a0[i] - t[i]) % r for i in range(s)]
    else:
        big, small = step_split(m)
        omega = root_of_unity(curve, 1 << clog2(m))
        u0, u1 = _radix2(curve, True, v[:big]), _radix2(curve, True, v[big:])
        tmp = [x * w % r for x, w in zip(u0, _powers(omega, big, r))]
        half = pow(2, -1, r)
        a = list(u0) + [0] * small
        for i, wi in enumerate(_powers(pow(omega, -1, r), small, r)):
            x = (u1[i] - sum(tmp[i + small::small])) * wi % r
            a[i] = (u0[i] + x) * half % r
            a[big + i] = (u0[i] - x) * half % r
    if coset:
        a = [x * gk % r for x, gk in zip(a, _powers(pow(G, -1, r), m, r))]
    return a


def z_on_coset_inverses(curve, kind, m):
    """1 / Z(g * element(idx)) for every idx: the same formula as `vanishing`, with the powers of g * element(idx) taken as running
    products along each part of the domain and one modular inversion per distinct value"""
    r = MODULUS[curve]
    A, B, C = _vanishing_form(curve, kind, m)
    n0, w0, off, w1 = _parts(curve, kind, m)
    cache, out = {}, []
    for first, step, n in ((G, w0, n0), (G * off % r, w1, m - n0)):
        ta, tb = pow(first, A, r), pow(first, B, r)
        sa, sb = pow(step, A, r), pow(step, B, r)
        for _ in range(n):
            z = (ta - 1) * (tb - C) % r
            if z not in cache:
                cache[z] = pow(z, -1, r)
            out.append(cache[z])
            ta, tb = ta * sa % r, tb * sb % r
    return out


def fast_compute_h_steps(curve, kind, m, ca, cb, cc):
    """compute_H on wire arrays [m, 12], every stage kept, as lists of Montgomery integers (x R mod r):
    coef = iFFT(x) and cos = cosetFFT(coef) for x in (ca, cb, cc); t = (a b - c) / Z on the coset; h = icosetFFT(t)"""
    r = MODULUS[curve]
    rinv = pow(R, -1, r)
    coef = [fast_ifft(curve, kind, m, mont_ints(x)) for x in (ca, cb, cc)]
    cos = [fast_fft(curve, kind, m, x, True) for x in coef]
    zinv = z_on_coset_inverses(curve, kind, m)
    t = [(x * y * rinv - z) * zi % r for x, y, z, zi in zip(cos[0], cos[1], cos[2], zinv)]      # x y / R is the product's Montgomery form
    return dict(coef=coef, cos=cos, zinv=zinv, t=t, h=fast_ifft(curve, kind, m, t, True))


def fast_compute_h_wire(curve, kind, m, ca, cb, cc):
    """compute_H on wire arrays [m, 12] -> [m + 1, 12]: x -> cosetFFT(iFFT(x)) for a, b, c; (a b - c) / Z; icosetFFT; a zero behind"""
    return ints_to_words(fast_compute_h_steps(curve, kind, m, ca, cb, cc)["h"] + [0])
