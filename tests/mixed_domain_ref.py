"""Python-integer checker for the mixed-radix evaluation domains of MNT6753, m = 2^a 5^b (TEST INFRASTRUCTURE).

The domain BY DEFINITION is tests/domain_ref.py's with kind = D.BASIC: its root_of_unity, element, fft_def, fft_at and vanishing
follow libff's get_root_of_unity through the small subgroup of Fr, so FFT(a)[k] = sum_i a[i] omega^(i k) there for every 2^a 5^b.

The `fast_*` functions here are the O(m log m) composition for sizes where O(m^2) integers are too slow: with m = Q T, Q = 5^b,
T = 2^a, i = i1 + Q i2 and k = T k1 + k2,
    X[T k1 + k2] = sum_{i1 < Q} omega^(i1 k2) (omega^T)^(i1 k1) Y_i1[k2],     Y_i1 = radix-2 FFT of (x[i1 + Q i2])_i2 with root omega^Q
-- the Q-axis in Python integers, the radix-2 part through the oracle (omega^Q is the basic domain's own root of unity of order T:
asserted).  tests/test_mixed_domains_cpu.py pins them to the definition at small sizes.  Elements are Python integers as in domain_ref.
"""
import domain_ref as D

CURVE = 1          # MNT6753: the only Fr of the cycle with a small subgroup
KIND_CODE = 3      # MNT753_DOMAIN_MIXED


def split(m):
    """m = Q T -> (Q, T), Q the power of 5 in m"""
    q = 1
    while m % 5 == 0:
        m //= 5
        q *= 5
    assert D.is_pow2(m)
    return q, m


def is_mixed_size(m):
    """what mnt753_domain_create_mixed accepts: 2^a 5^b, a <= 15, 1 <= b <= 2"""
    if m <= 0 or m % 5:
        return False
    q = 1
    while m % 5 == 0:
        m //= 5
        q *= 5
    return q <= 25 and D.is_pow2(m) and m <= 1 << 15


def _inner_root_checked(m):
    q, t = split(m)
    r = D.MODULUS[CURVE]
    w = D.root_of_unity(CURVE, m)
    if t > 1:
        assert pow(w, q, r) == D.root_of_unity(CURVE, t), "omega^Q is not the radix-2 domain's root"
    return w, q, t


def _transform(m, x, inverse):
    """sum_i x[i] w^(i k) for w = omega (or omega^-1; the inverse's 1 / m included)"""
    r = D.MODULUS[CURVE]
    w, q, t = _inner_root_checked(m)
    if inverse:
        w = pow(w, -1, r)
    # the oracle's inverse transform carries 1 / T: the remaining 1 / Q is applied below
    ys = [D._radix2(CURVE, inverse, list(x[i1::q])) for i1 in range(q)]
    wk2 = D._powers(w, t, r)                      # omega^k2
    zq = D._powers(pow(w, t, r), q, r)            # (omega^T)^e, e < Q: a Q-th root of unity
    scale = pow(q, -1, r) if inverse else 1
    out = [0] * m
    for k2 in range(t):
        tw = D._powers(wk2[k2], q, r)             # omega^(i1 k2)
        terms = [tw[i1] * ys[i1][k2] % r for i1 in range(q)]
        for k1 in range(q):
            out[t * k1 + k2] = sum(zq[i1 * k1 % q] * terms[i1] for i1 in range(q)) * scale % r
    return out


def fast_fft(m, a, coset=False):
    r = D.MODULUS[CURVE]
    if coset:
        a = [v * gk % r for v, gk in zip(a, D._powers(D.G, m, r))]
    return _transform(m, a, False)


def fast_ifft(m, v, coset=False):
    r = D.MODULUS[CURVE]
    a = _transform(m, v, True)
    if coset:
        a = [x * gk % r for x, gk in zip(a, D._powers(pow(D.G, -1, r), m, r))]
    return a


def z_inverse(m):
    """1 / Z(g x) on the coset: Z(t) = t^m - 1 is the one constant g^m - 1 there"""
    r = D.MODULUS[CURVE]
    return pow(pow(D.G, m, r) - 1, -1, r)


def fast_compute_h_steps(m, ca, cb, cc):
    """compute_H on wire arrays [m, 12], every stage kept, as lists of Montgomery integers (as domain_ref.fast_compute_h_steps)"""
    r = D.MODULUS[CURVE]
    rinv = pow(D.R, -1, r)
    coef = [fast_ifft(m, D.mont_ints(x)) for x in (ca, cb, cc)]
    cos = [fast_fft(m, x, True) for x in coef]
    zi = z_inverse(m)
    t = [(x * y * rinv - z) * zi % r for x, y, z in zip(cos[0], cos[1], cos[2])]
    return dict(coef=coef, cos=cos, zinv=zi, t=t, h=fast_ifft(m, t, True))


def fast_compute_h(m, ca, cb, cc):
    """compute_H on wire arrays [m, 12] -> [m + 1, 12]"""
    return D.ints_to_words(fast_compute_h_steps(m, ca, cb, cc)["h"] + [0])
