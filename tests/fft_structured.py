"""Structured inputs of the radix-2 transforms and their EXACT transforms as closed forms (TEST INFRASTRUCTURE).

Uniform random vectors sit mid-range in the carry-free butterflies of k_ntt_group and never give an output that is 0 mod r.  The
vectors here do: their transforms are mostly zeros (constant, alternating, periodic vectors), or every operand is pinned at the
largest canonical word pattern r - 1.  Each class comes with the closed form of FFT, iFFT, cosetFFT and icosetFFT on the basic
radix-2 domain of size m (libfqfft's basic_radix2_domain: omega the primitive m-th root, g the multiplicative generator):

    FFT(a)[k] = sum_i a_i omega^(ik)      iFFT(a)[k] = (1/m) sum_i a_i omega^(-ik)
    cosetFFT(a) = FFT(a_i g^i)            icosetFFT(a)[k] = g^(-k) iFFT(a)[k]

The closed forms share nothing with a butterfly network: geometric sums, powers of omega, and -- for the periodic and the
zero-stuffed class -- a transform of the SHORT seed vector (small_fft below, n <= 2^10 elements).  tests/test_fft_structured_cpu.py
pins every one of them to the oracle for every log2 m <= 12 on both curves.

All vectors are lists of Python integers holding the RAW wire value of each element (x R mod r, R = 2^768, what the 12 words of the
ABI spell): the four transforms are linear, so they act on the Montgomery integers exactly as on the values, and "r - 1" below is
the word pattern r - 1 itself, the largest a canonical element can have.  `words` turns a list into the ABI's uint64 [m, 12].
"""
import random

import domain_ref as D

FFT, IFFT, COSET_FFT, ICOSET_FFT = 0, 1, 2, 3
KINDS = (FFT, IFFT, COSET_FFT, ICOSET_FFT)
words = D.ints_to_words
ints = D.mont_ints


def modulus(curve):
    return D.MODULUS[curve]


def mont_one(curve):
    return D.R % D.MODULUS[curve]


def seeded(curve, seed, n):
    """n raw values in [0, r) from a seed (Python's Mersenne twister: the same on every platform)"""
    rng = random.Random(0x66667473 + 1000003 * seed + curve)
    return [rng.randrange(D.MODULUS[curve]) for _ in range(n)]


def mont_mul(curve, x, y):
    """the raw value of the field product of two raw values: x y / R"""
    r = D.MODULUS[curve]
    return x * y * pow(D.R, -1, r) % r


def batch_inverse(xs, r):
    """1 / x for every x (none zero mod r): one modular inversion for the list"""
    pre, acc = [], 1
    for x in xs:
        pre.append(acc)
        acc = acc * x % r
    inv = pow(acc, -1, r)
    out = [0] * len(xs)
    for i in range(len(xs) - 1, -1, -1):
        out[i] = inv * pre[i] % r
        inv = inv * xs[i] % r
    return out


def small_fft(curve, s, inverse=False):
    """The size-n transform of a short vector by the Cooley-Tukey recursion FFT(s)[k] = E[k mod n/2] + w^k O[k mod n/2] (even and
    odd halves), with its 1/n for the inverse.  n = len(s) is a power of two; n = 1 is the identity."""
    r = D.MODULUS[curve]
    n = len(s)
    if n == 1:
        return list(s)
    w = D.root_of_unity(curve, n)
    if inverse:
        w = pow(w, -1, r)

    def rec(v, wn):
        if len(v) == 1:
            return v
        even, odd = rec(v[0::2], wn * wn % r), rec(v[1::2], wn * wn % r)
        h, out, t = len(v) // 2, [0] * len(v), 1
        for k in range(h):
            x = t * odd[k] % r
            out[k], out[k + h] = (even[k] + x) % r, (even[k] - x) % r
            t = t * wn % r
        return out

    out = rec(list(s), w)
    if inverse:
        ninv = pow(n, -1, r)
        out = [x * ninv % r for x in out]
    return out


# ---- the classes -----------------------------------------------------------------------------------------------------------------
# A spec is a tuple: ("zero",) | ("const", c) | ("delta", j, v) | ("alt", c) | ("periodic", s) | ("stuffed", s)
def build(curve, m, spec):
    """the input vector of a spec: m raw values"""
    r = D.MODULUS[curve]
    tag = spec[0]
    if tag == "zero":
        return [0] * m
    if tag == "const":
        return [spec[1] % r] * m
    if tag == "delta":
        v = [0] * m
        v[spec[1]] = spec[2] % r
        return v
    if tag == "alt":                           # (c, r - c, c, r - c, ...): c (-1)^i
        c = spec[1] % r
        return [c, (r - c) % r] * (m // 2)
    if tag == "periodic":                      # a_i = s_(i mod n)
        s = spec[1]
        return list(s) * (m // len(s))
    if tag == "stuffed":                       # a_(j m/n) = s_j, zero elsewhere
        s = spec[1]
        v = [0] * m
        v[::m // len(s)] = s
        return v
    raise ValueError(tag)


def transform(curve, kind, m, spec):
    """the exact transform of build(curve, m, spec): m raw values.  m >= 2, a power of two."""
    r = D.MODULUS[curve]
    g = D.G
    w = D.root_of_unity(curve, m)
    winv, ginv, minv = pow(w, -1, r), pow(g, -1, r), pow(m, -1, r)
    gm1 = (pow(g, m, r) - 1) % r               # g^m - 1: the numerator of every geometric sum over the coset
    tag = spec[0]
    zeros = [0] * m
    if tag == "zero":
        return zeros
    if tag == "const":                         # sum_i x^i = (x^m - 1) / (x - 1); x = omega^k: m at k = 0, else 0
        c = spec[1] % r
        if kind == COSET_FFT:                  # x = g omega^k: never 1
            den = batch_inverse([(gw - 1) % r for gw in D._powers(w, m, r, g)], r)
            return [c * gm1 % r * d % r for d in den]
        zeros[0] = c * m % r if kind == FFT else c
        return zeros
    if tag == "delta":                         # one term: v x^j
        j, v = spec[1], spec[2] % r
        if kind == FFT:
            return D._powers(pow(w, j, r), m, r, v)
        if kind == IFFT:
            return D._powers(pow(winv, j, r), m, r, v * minv)
        if kind == COSET_FFT:
            return D._powers(pow(w, j, r), m, r, v * pow(g, j, r))
        return D._powers(pow(winv, j, r) * ginv % r, m, r, v * minv)
    if tag == "alt":                           # a_i = c omega^(i m/2): the FFT of a character is m at its own index
        c, h = spec[1] % r, m // 2
        if kind == COSET_FFT:                  # sum_i (-g omega^k)^i = ((-g)^m - 1) / (-g omega^k - 1), m even
            den = batch_inverse([(-gw - 1) % r for gw in D._powers(w, m, r, g)], r)
            return [c * gm1 % r * d % r for d in den]
        zeros[h] = {FFT: c * m % r, IFFT: c, ICOSET_FFT: c * pow(ginv, h, r) % r}[kind]
        return zeros
    s = [x % r for x in spec[1]]
    n = len(s)
    t = m // n
    if tag == "periodic":
        if kind != COSET_FFT:
            zeros[::t] = periodic_values(curve, kind, m, s)
            return zeros
        # cosetFFT: sum_i s_(i mod n) x^i = S(x) (x^m - 1) / (x^n - 1) at x = g omega^k, S the short polynomial; x^n = g^n (omega^n)^k
        # takes t values.  O(m n): for short seeds
        if t == 1:
            geo = [1]
        else:
            geo = [gm1 * d % r for d in batch_inverse([(xn - 1) % r for xn in D._powers(pow(w, n, r), t, r, pow(g, n, r))], r)]
        return [D._horner(s, x, r) * geo[k % t] % r for k, x in enumerate(D._powers(w, m, r, g))]
    if tag == "stuffed":
        if kind != ICOSET_FFT:
            return stuffed_block(curve, kind, m, s) * t
        return [x * gk % r for x, gk in zip(stuffed_block(curve, IFFT, m, s) * t, D._powers(ginv, m, r))]
    raise ValueError(tag)


def periodic_values(curve, kind, m, s):
    """FFT, iFFT or icosetFFT of the period-n extension of s (n = len(s)) to m elements: the n outputs at the multiples of
    t = m / n; every other output is 0 (sum_q omega^(k n q) is t where t divides k, else 0).  O(n log n) whatever m is."""
    r = D.MODULUS[curve]
    n = len(s)
    t = m // n
    if kind == FFT:
        return [x * t % r for x in small_fft(curve, s)]
    if kind == IFFT:
        return small_fft(curve, s, True)
    if kind == ICOSET_FFT:
        return [x * gk % r for x, gk in zip(small_fft(curve, s, True), D._powers(pow(D.G, -t, r), n, r))]
    raise ValueError(kind)


def stuffed_block(curve, kind, m, s):
    """FFT, iFFT or cosetFFT of the zero-stuffed s (a_(j t) = s_j, t = m / n): sum_j s_j x^(j t) is a size-n transform in x^t, so
    the m outputs are this block of n repeated t times.  O(n log n) whatever m is."""
    r = D.MODULUS[curve]
    n = len(s)
    t = m // n
    if kind == FFT:
        return small_fft(curve, s)
    if kind == IFFT:
        tinv = pow(t, -1, r)
        return [x * tinv % r for x in small_fft(curve, s, True)]
    if kind == COSET_FFT:
        return small_fft(curve, [x * gk % r for x, gk in zip(s, D._powers(pow(D.G, t, r), n, r))])
    raise ValueError(kind)


def schedule(logm, max_ns=8):
    """The LDS groups k_ntt_group runs a size-2^logm transform in: ceil(logm / 8) launches of balanced width (run_stages)"""
    groups = (logm + max_ns - 1) // max_ns
    out, s0 = [], 0
    for gi in range(groups):
        ns = (logm - s0 + (groups - gi) - 1) // (groups - gi)
        out.append(ns)
        s0 += ns
    return out


def classes(curve, m, seed=1, n=4):
    """[(name, spec)]: every class of the module at size m (m >= 2).  n: the seed length of the periodic and zero-stuffed classes
    (cut to m).  "r - 1" is the word pattern; "-1" the field's minus one, whose words are r - (R mod r)."""
    r = D.MODULUS[curve]
    sd = seeded(curve, seed, 2 + 2 * n)
    c, c2, small_p, small_s = sd[0], sd[1], sd[2:2 + min(n, m)], sd[2 + n:2 + n + min(n, m)]
    small_p = small_p[:-1] + [r - 1]           # one element of the seed vector at the edge as well
    out = [("zero", ("zero",)),
           ("const-one", ("const", mont_one(curve))), ("const-r-1", ("const", r - 1)), ("const-minus-one", ("const", r - mont_one(curve))),
           ("const-seeded", ("const", c))]
    for j in sorted({0, m // 2, m - 1}):
        out.append((f"delta-r-1-at-{j}", ("delta", j, r - 1)))
    out += [("alt-seeded", ("alt", c2)), ("alt-r-1", ("alt", r - 1)),
            (f"periodic-{len(small_p)}", ("periodic", small_p)), (f"stuffed-{len(small_s)}", ("stuffed", small_s))]
    return out


# ---- compute_H ---------------------------------------------------------------------------------------------------------------------
# Rows (ca_i, cb_i, cc_i = ca_i cb_i) are all satisfied: A B - C vanishes on the domain, so the pointwise step of compute_H sees
# the coset values of a multiple of Z and the quotient H = (A B - C) / Z has degree < m - 1.  Three pairs have H in closed form:
#   const x const:   A, B, C are constants, A B - C = 0:                     H = 0
#   alt c x alt d:   A = c x^(m/2), B = d x^(m/2), C = c d:  A B - C = c d Z:  H = c d
#   delta x delta (both at j, values v, u): A = v L_j, B = u L_j, C = v u L_j with L_j = (omega^j / m) Z / (x - omega^j):
#                    H = v u (omega^j / m) (L_j - 1) / (x - omega^j) = (v u / m^2) sum_(l <= m - 2) (m - 1 - l) omega^(-j l) x^l
def product_rows(curve, a, b):
    r = D.MODULUS[curve]
    rinv = pow(D.R, -1, r)
    return [x * y * rinv % r for x, y in zip(a, b)]


def compute_h_closed(curve, m, spec_a, spec_b):
    """h (m + 1 raw values) of compute_H on (build(spec_a), build(spec_b), their row products), for the three pairs above"""
    r = D.MODULUS[curve]
    ta, tb = spec_a[0], spec_b[0]
    h = [0] * (m + 1)
    if ta == "const" and tb == "const":
        return h
    if ta == "alt" and tb == "alt":
        h[0] = mont_mul(curve, spec_a[1] % r, spec_b[1] % r)
        return h
    if ta == "delta" and tb == "delta" and spec_a[1] == spec_b[1]:
        j = spec_a[1]
        k = mont_mul(curve, spec_a[2] % r, spec_b[2] % r) * pow(m * m, -1, r) % r
        wj = D._powers(pow(D.root_of_unity(curve, m), -j, r), m - 1, r)
        h[:m - 1] = [k * (m - 1 - l) % r * wj[l] % r for l in range(m - 1)]
        return h
    raise ValueError((ta, tb))


def h_pairs(curve, m, seed=1, n=4):
    """[(name, spec_a, spec_b, closed)]: the pairs compute_H is run on; closed says compute_h_closed knows the answer"""
    r = D.MODULUS[curve]
    cl = dict(classes(curve, m, seed, n))
    per, stu = (v for k, v in cl.items() if k.startswith("periodic")), (v for k, v in cl.items() if k.startswith("stuffed"))
    per, stu = next(per), next(stu)
    return [("const-r-1 x const-r-1", cl["const-r-1"], cl["const-r-1"], True),
            ("const-seeded x const-minus-one", cl["const-seeded"], cl["const-minus-one"], True),
            ("alt-r-1 x alt-seeded", cl["alt-r-1"], cl["alt-seeded"], True),
            (f"delta-r-1-at-{m - 1} twice", ("delta", m - 1, r - 1), ("delta", m - 1, r - 1), True),
            ("delta-r-1-at-0 x delta-seeded-at-0", ("delta", 0, r - 1), ("delta", 0, cl["const-seeded"][1]), True),
            ("periodic x stuffed", per, stu, False),
            ("const-r-1 x periodic", cl["const-r-1"], per, False),
            ("zero x const-seeded", cl["zero"], cl["const-seeded"], False)]
