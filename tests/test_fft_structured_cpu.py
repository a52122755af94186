"""CPU: the closed forms of tests/fft_structured.py are what the reference computes -- every class, every transform kind and the
three compute_H pairs against the oracle (oracle/liboracle.so: libfqfft's serial radix-2 FFT restated), on both curves, for every
log2 m <= 12.  This pins the expectations tests/test_fft_schedules_gpu.py holds the kernels to on a machine without a GPU."""
import numpy as np
import pytest

import fft_structured as S
import oracle_lib as O

LOGM = range(1, 13)


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("logm", LOGM)
def test_closed_forms_equal_the_oracle(curve, logm):
    m = 1 << logm
    # seed lengths 4 and (where they fit) 16 and 2^10: the period / stride of the last two classes at both ends of what the GPU tests use
    seen = set()
    for n in (4, 16, 1 << 10):
        for name, spec in S.classes(curve, m, seed=logm, n=n):
            if name in seen or (n > 16 and spec[0] == "periodic"):      # the periodic cosetFFT form costs m n: short seeds only
                continue
            seen.add(name)
            v = S.words(S.build(curve, m, spec))
            for kind in S.KINDS:
                want = O.fft(curve, kind, v).reshape(m, 12)
                assert np.array_equal(S.words(S.transform(curve, kind, m, spec)), want), f"{name}, kind {kind}"


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("logm", [1, 5, 10])
def test_long_period_plain_transforms(curve, logm):
    """period 2^10 (cut to m) through FFT, iFFT and icosetFFT: the forms the 2^21 ... 2^25 cases use"""
    m = 1 << logm
    name, spec = [c for c in S.classes(curve, m, seed=77, n=1 << 10) if c[1][0] == "periodic"][0]
    v = S.words(S.build(curve, m, spec))
    for kind in (S.FFT, S.IFFT, S.ICOSET_FFT):
        assert np.array_equal(S.words(S.transform(curve, kind, m, spec)), O.fft(curve, kind, v).reshape(m, 12)), f"{name}, kind {kind}"


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("logm", LOGM)
def test_compute_h_closed_forms_equal_the_oracle(curve, logm):
    m = 1 << logm
    r = S.modulus(curve)
    for name, sa, sb, closed in S.h_pairs(curve, m, seed=logm):
        a, b = S.build(curve, m, sa), S.build(curve, m, sb)
        c = S.product_rows(curve, a, b)
        # the rows are satisfied in the oracle's own arithmetic (field_op 0 is the product)
        for i in sorted({0, 1, m // 2, m - 1}):
            assert S.ints(O.field_op(curve, 0, S.words([a[i]])[0], S.words([b[i]])[0]))[0] == c[i] < r
        h = O.compute_h(curve, S.words(a), S.words(b), S.words(c)).reshape(m + 1, 12)
        if closed:
            assert np.array_equal(S.words(S.compute_h_closed(curve, m, sa, sb)), h), name
        assert not h[m].any() and not h[m - 1].any(), name      # deg H <= m - 2


def test_small_fft_is_the_oracle_fft():
    for curve in (0, 1):
        for n in (1, 2, 8, 1 << 10):
            s = S.seeded(curve, 5, n)
            if n == 1:
                assert S.small_fft(curve, s) == s and S.small_fft(curve, s, True) == s
                continue
            for inverse in (False, True):
                assert np.array_equal(S.words(S.small_fft(curve, s, inverse)), O.fft(curve, 1 if inverse else 0, S.words(s)).reshape(n, 12))


def test_schedules_the_gpu_cases_cover():
    """what tests/test_fft_schedules_gpu.py promises about its sizes: every width 1 ... 8 as a first group, 5 ... 8 as a last group
    behind another one, three- and four-group schedules, and the splits its docstring lists"""
    sched = {logm: S.schedule(logm) for logm in range(1, 26)}
    assert all(sum(s) == logm and max(s) <= 8 and len(s) == -(-logm // 8) for logm, s in sched.items())
    assert {s[0] for s in sched.values()} == set(range(1, 9))
    assert {s[-1] for s in sched.values() if len(s) > 1} >= {5, 6, 7, 8}
    assert {len(s) for s in sched.values()} == {1, 2, 3, 4}
    assert (sched[11], sched[17], sched[21], sched[24], sched[25]) == ([6, 5], [6, 6, 5], [7, 7, 7], [8, 8, 8], [7, 6, 6, 6])
