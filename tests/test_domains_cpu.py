"""CPU: pins tests/domain_ref.py -- the checker the GPU domain tests compare against -- without a GPU.

* at every power of two of the committed golden vectors (fft_mnt{4,6}_*.bin, h_mnt{4,6}_*.bin, written by libfqfft itself) the
  definitions and the fast composition reproduce the reference word for word;
* for step and extended sizes the fast composition equals the definition, iFFT(FFT(v)) == v, and divide_by_Z_on_coset by running
  products equals the vanishing polynomial evaluated point by point;
* `select` gives the table of the walk of get_evaluation_domain (a model written from the reference's code; the minted
  tests/golden/domains/hashes.json records what the reference binary did for three of its rows);
* without a device mnt753_domain_create_for refuses like its sibling."""
import ctypes
import random

import numpy as np
import pytest

import domain_ref as D
import golden_io as G


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("logm", G.FFT_LOGM)
def test_reproduces_golden_fft(curve, logm):
    m = 1 << logm
    assert D.select(curve, m) == (D.BASIC, m)
    v, outs = G.fft(curve, logm)
    a = D.from_wire(curve, v)
    assert np.array_equal(D.to_wire(curve, D.fft_def(curve, D.BASIC, m, a)), outs[0])
    assert np.array_equal(D.to_wire(curve, D.fft_def(curve, D.BASIC, m, a, coset=True)), outs[2])
    assert D.is_ifft_of(curve, D.BASIC, m, D.from_wire(curve, outs[1]), a)
    assert D.is_ifft_of(curve, D.BASIC, m, D.from_wire(curve, outs[3]), a, coset=True)
    # the fast composition works on the Montgomery integers themselves
    raw = D.mont_ints(v)
    assert np.array_equal(D.ints_to_words(D.fast_fft(curve, D.BASIC, m, raw)), outs[0])
    assert np.array_equal(D.ints_to_words(D.fast_ifft(curve, D.BASIC, m, raw)), outs[1])
    assert np.array_equal(D.ints_to_words(D.fast_fft(curve, D.BASIC, m, raw, coset=True)), outs[2])
    assert np.array_equal(D.ints_to_words(D.fast_ifft(curve, D.BASIC, m, raw, coset=True)), outs[3])


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("logm", G.H_LOGM)
def test_reproduces_golden_compute_h(curve, logm):
    ca, cb, cc, h = G.h(curve, logm)
    assert np.array_equal(D.fast_compute_h_wire(curve, D.BASIC, 1 << logm, ca, cb, cc), h)
    # divide_by_Z_on_coset of a basic domain: one constant, 1 / (g^m - 1)
    m, r = 1 << logm, D.MODULUS[curve]
    assert set(D.z_on_coset_inverses(curve, D.BASIC, m)) == {pow(pow(D.G, m, r) - 1, -1, r)}


CASES = ([(0, D.STEP, m) for m in (3, 5, 6, 12, 24, 40, 96, 1040, 1536)] + [(1, D.STEP, m) for m in (3, 6, 12, 24, 96, 1040, 1536)] +
         # the extended domain exists at 2^(s+1) only; the checker's formulas do not depend on that, so they are pinned where O(m^2) is cheap
         [(0, D.EXTENDED, 8), (1, D.EXTENDED, 64), (1, D.EXTENDED, 512)])


@pytest.mark.parametrize("curve,kind,m", CASES)
def test_fast_composition_equals_the_definition(curve, kind, m):
    r = D.MODULUS[curve]
    rng = random.Random(1000 * m + curve)
    v = [rng.randrange(r) for _ in range(m)]
    xs = D.elements(curve, kind, m)
    assert len(set(xs)) == m and xs == [D.element(curve, kind, m, i) for i in range(m)]
    assert all(D.vanishing(curve, kind, m, x) == 0 for x in xs)                 # Z is zero on the domain ...
    assert all(D.vanishing(curve, kind, m, D.G * x % r) != 0 for x in xs)       # ... and nowhere on the coset
    for coset in (False, True):
        f = D.fft_def(curve, kind, m, v, coset)
        assert D.fast_fft(curve, kind, m, v, coset) == f
        assert D.fast_ifft(curve, kind, m, f, coset) == v                       # iFFT(FFT(v)) == v
        assert D.is_ifft_of(curve, kind, m, D.fast_ifft(curve, kind, m, v, coset), v, coset)
    zi = D.z_on_coset_inverses(curve, kind, m)
    assert [p * z % r for p, z in zip(v, zi)] == D.divide_by_z_on_coset_def(curve, kind, m, v)
    distinct = len(set(zi))
    assert distinct <= (2 if kind == D.EXTENDED else D.step_split(m)[0] // D.step_split(m)[1] + 1)


@pytest.mark.parametrize("curve,kind,m", [(0, D.STEP, 24), (1, D.STEP, 96), (0, D.STEP, 5), (1, D.EXTENDED, 64)])
def test_compute_h_composition_satisfies_the_definition(curve, kind, m):
    """H(x) Z(x) = A(x) B(x) - C(x) on the coset, A, B, C the interpolants of ca, cb, cc on the domain"""
    r = D.MODULUS[curve]
    rng = random.Random(7 * m + curve)
    plain = [[rng.randrange(r) for _ in range(m)] for _ in range(3)]
    h = D.from_wire(curve, D.fast_compute_h_wire(curve, kind, m, *(D.to_wire(curve, v) for v in plain)))
    assert h[m] == 0
    A, B, C = (D.fast_ifft(curve, kind, m, v) for v in plain)
    for x in D.elements(curve, kind, m):
        t = D.G * x % r
        assert D._horner(h[:m], t, r) * D.vanishing(curve, kind, m, t) % r == (D._horner(A, t, r) * D._horner(B, t, r) - D._horner(C, t, r)) % r


def test_eval_many_matches_horner():
    r = D.MODULUS[0]
    rng = random.Random(3)
    polys = [[rng.randrange(r) for _ in range(n)] for n in (1, 7, 1024, 1025, 3000)]
    tasks = [(k, rng.randrange(r)) for k in range(len(polys)) for _ in range(2)]
    naive = lambda p, x: sum(c * pow(x, i, r) for i, c in enumerate(p)) % r
    assert D.eval_many(polys, tasks, r) == [naive(polys[k], x) for k, x in tasks]


P = lambda *e: sum(1 << x for x in e)
TABLE = {
    0: [(m, D.STEP, m) for m in (3, 5, 6, 12, 24, 40, 96, 1040, 1536, P(19, 18))] + [(21, D.STEP, 24), (25, D.BASIC, 32), (50000, D.BASIC, 1 << 16)] +
       [(1 << k, D.BASIC, 1 << k) for k in range(1, 31)] + [(0, D.NONE, 0), (1, D.NONE, 0)],
    1: [(m, D.STEP, m) for m in (3, 6, 12, 24, 96, 1040, 1536, P(13, 10), P(14, 13))] + [(1 << 16, D.EXTENDED, 1 << 16), (21, D.STEP, 24)] +
       [(P(15, 14) + 1, D.EXTENDED, 1 << 16), (50000, D.EXTENDED, 1 << 16)] + [(1 << k, D.BASIC, 1 << k) for k in range(1, 16)] +
       # the reference stops at a mixed-radix basic domain (candidate 1) ...
       [(m, D.MIXED, m) for m in (5, 10, 25, 40, 5 << 15)] +
       # ... or at candidate 7's best mixed size: 25 * 2^11, 5 * 2^15, 25 * 2^15 ...
       [(P(15, 14), D.MIXED, 25 << 11), (1 << 17, D.MIXED, 5 << 15), (P(19, 18), D.MIXED, 25 << 15)] +
       # ... or goes past it
       [(1 << 20, D.SEQUENCE, 1 << 20), (0, D.NONE, 0), (1, D.NONE, 0)],
}


@pytest.mark.parametrize("curve", [0, 1])
def test_selection_table(curve):
    for min_size, kind, m in TABLE[curve]:
        assert D.select(curve, min_size) == (kind, m), (curve, min_size)


def test_every_5_times_power_of_two_is_mixed_on_mnt6753():
    """2^k + 2^(k-2) looks like a step size; on MNT6753 the reference's basic domain takes it first"""
    for k in range(2, 16):
        m = (1 << k) + (1 << (k - 2))
        assert D.select(1, m) == (D.MIXED, m) and D.select(0, m) == (D.STEP, m)


def test_create_for_without_a_device(pkg):
    """no silent fallback: like mnt753_domain_create, mnt753_domain_create_for answers MNT753_ENODEV before a device is initialised"""
    try:
        import torch
        if torch.cuda.is_available():
            pytest.skip("a GPU is present: the library initialises")
    except ImportError:
        pass
    L = ctypes.CDLL(pkg.lib_path())
    L.mnt753_domain_create_for.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p)]
    L.mnt753_domain_create.argtypes = L.mnt753_domain_create_for.argtypes
    L.mnt753_domain_kind.argtypes = [ctypes.c_void_p]
    h = ctypes.c_void_p()
    for m in (24, 1 << 10, 5):
        assert L.mnt753_domain_create_for(0, m, ctypes.byref(h)) == -2     # MNT753_ENODEV
    assert L.mnt753_domain_create(0, 1 << 10, ctypes.byref(h)) == -2
    assert L.mnt753_domain_kind(None) == -1
