"""GPU: evaluation domains beyond powers of two (mnt753_domain_create_for: extended and step radix-2), element-wise and bit-exact
against tests/domain_ref.py.

Every step size of the selection table up to 1536 is checked at EVERY output index against the definition (the polynomial's values at
the domain's elements; an inverse transform by evaluating its result).  The four sizes where O(m^2) integers are too slow compare the
whole vector with domain_ref's fast composition (its O(m) passes in Python around the oracle's radix-2 FFT, pinned to the definition
by tests/test_domains_cpu.py) and with the definition at 64 seeded output indices; that sample is the only thinning."""
import random

import numpy as np
import pytest

import domain_ref as D

pytestmark = pytest.mark.gpu

STEP_SMALL = {0: [3, 5, 6, 12, 24, 40, 96, 1040, 1536], 1: [3, 6, 12, 24, 96, 1040, 1536]}
LARGE = [(1, D.EXTENDED, 1 << 16), (1, D.STEP, (1 << 13) + (1 << 10)), (1, D.STEP, (1 << 14) + (1 << 13)), (0, D.STEP, (1 << 19) + (1 << 18))]
N_SAMPLES = 64


def words(ints):
    return D.ints_to_words(ints)


def on_gpu(gpu, vec, fn):
    """fn(device pointer) on a device copy of the wire array vec -> the array afterwards"""
    buf = gpu.DeviceBuffer.from_numpy(np.ascontiguousarray(vec, dtype=np.uint64))
    fn(buf.ptr.value)
    out = buf.to_numpy().reshape(-1, 12)
    buf.close()
    return out


def check_domain(gpu, curve, kind, m, idxs):
    """All entry points of one domain.  Whole vectors against the fast composition; the definition at the output indices idxs."""
    r = D.MODULUS[curve]
    rinv = pow(D.R, -1, r)
    dom = gpu.Domain.for_size(curve, m)
    assert (dom.kind, dom.m) == (D.KIND_CODE[kind], m)
    ca, cb, cc = (gpu.synth_scalars(curve, 700 + i, m) for i in range(3))
    st = D.fast_compute_h_steps(curve, kind, m, ca, cb, cc)
    A, B, Cc = st["coef"]
    vin = [D.mont_ints(x) for x in (ca, cb, cc)]
    # the definition at the indices idxs: A, B, C, H as polynomials, evaluated at element(idx) and at g * element(idx)
    idxs = list(idxs)
    polys = [A, B, Cc, st["h"]]
    xs = [D.element(curve, kind, m, i) for i in idxs]
    tasks = [(k, x) for x in xs for k in (0, 1, 2)] + [(k, D.G * x % r) for x in xs for k in (0, 1, 2, 3)]
    vals = D.eval_many(polys, tasks, r)
    plain = {(k, i): vals[3 * n + k] for n, i in enumerate(idxs) for k in (0, 1, 2)}
    coset = {(k, i): vals[3 * len(idxs) + 4 * n + k] for n, i in enumerate(idxs) for k in (0, 1, 2, 3)}
    zs = {i: D.vanishing(curve, kind, m, D.G * x % r) for i, x in zip(idxs, xs)}

    # iFFT: the result, evaluated at the domain's elements, is the input
    got = on_gpu(gpu, ca, lambda p: dom.fft(gpu.IFFT, p))
    assert np.array_equal(got, words(A)), "iFFT"
    assert all(plain[k, i] == vin[k][i] for i in idxs for k in (0, 1, 2)), "iFFT against the definition"
    # FFT: the polynomial's values at the domain's elements
    got = on_gpu(gpu, words(A), lambda p: dom.fft(gpu.FFT, p))
    assert np.array_equal(got, words(D.fast_fft(curve, kind, m, A))), "FFT"
    g = D.mont_ints(got)
    assert all(plain[0, i] == g[i] for i in idxs), "FFT against the definition"
    # cosetFFT: its values at g * element
    got = on_gpu(gpu, words(A), lambda p: dom.fft(gpu.COSET_FFT, p))
    assert np.array_equal(got, words(st["cos"][0])), "cosetFFT"
    g = D.mont_ints(got)
    assert all(coset[0, i] == g[i] for i in idxs), "cosetFFT against the definition"
    # icosetFFT: the result, evaluated at g * element, is the input
    got = on_gpu(gpu, words(st["t"]), lambda p: dom.fft(gpu.ICOSET_FFT, p))
    assert np.array_equal(got, words(st["h"])), "icosetFFT"
    assert all(coset[3, i] == st["t"][i] for i in idxs), "icosetFFT against the definition"
    # divide_by_Z_on_coset: by the vanishing polynomial at g * element(idx)
    got = on_gpu(gpu, ca, lambda p: dom.divide_by_z_on_coset(p))
    assert np.array_equal(got, words([v * zi % r for v, zi in zip(vin[0], st["zinv"])])), "divide_by_Z_on_coset"
    g = D.mont_ints(got)
    assert all(g[i] * zs[i] % r == vin[0][i] for i in idxs), "divide_by_Z_on_coset against the definition"
    # compute_H: H(x) Z(x) = A(x) B(x) - C(x) at x = g * element(idx), A, B, C the interpolants of ca, cb, cc (pinned above)
    a, b, c = (gpu.DeviceBuffer.from_numpy(x) for x in (ca, cb, cc))
    dh = gpu.DeviceBuffer(96 * (m + 1))
    dom.compute_h(a.ptr.value, b.ptr.value, c.ptr.value, dh.ptr.value)
    h = dh.to_numpy().reshape(m + 1, 12)
    assert np.array_equal(h, words(st["h"] + [0])), "compute_h"
    hp = D.mont_ints(h[:m])
    assert hp == st["h"]
    for i in idxs:       # coset[3, i] is the value at g * element(i) of the polynomial the GPU returned (hp == polys[3])
        assert coset[3, i] * zs[i] % r == (coset[0, i] * coset[1, i] * rinv - coset[2, i]) % r, "compute_h against the definition"
    # the split form (one chain per vector, then the join) gives the same words
    a2, b2, c2 = (gpu.DeviceBuffer.from_numpy(x) for x in (ca, cb, cc))
    for v in (a2, b2, c2):
        dom.compute_h_chain(v.ptr.value)
    assert np.array_equal(b2.to_numpy().reshape(m, 12), words(st["cos"][1])), "compute_h_chain"
    dh2 = gpu.DeviceBuffer(96 * (m + 1))
    dom.compute_h_finish(a2.ptr.value, b2.ptr.value, c2.ptr.value, dh2.ptr.value)
    assert np.array_equal(dh2.to_numpy().reshape(m + 1, 12), h), "compute_h_chain x3 + compute_h_finish"
    for x in (a, b, c, dh, a2, b2, c2, dh2):
        x.close()
    dom.close()


@pytest.mark.parametrize("curve,m", [(c, m) for c in (0, 1) for m in STEP_SMALL[c]])
def test_step_every_index(gpu, curve, m):
    assert D.select(curve, m) == (D.STEP, m)
    check_domain(gpu, curve, D.STEP, m, range(m))


@pytest.mark.parametrize("curve,m", [(0, 1025), (1, 1026)])
def test_step_with_a_long_fold(gpu, curve, m):
    """2^10 + 1 and 2^10 + 2 (not in the table): 1024 / 512 strided terms per output of the fold, summed by 256 / 128 threads each"""
    assert D.select(curve, m) == (D.STEP, m)
    check_domain(gpu, curve, D.STEP, m, range(m))


@pytest.mark.parametrize("curve,kind,m", LARGE)
def test_large_whole_vector_and_samples(gpu, curve, kind, m):
    assert D.select(curve, m) == (kind, m)
    rng = random.Random(0x646f6d + m)
    check_domain(gpu, curve, kind, m, sorted(rng.sample(range(m), N_SAMPLES)))


@pytest.mark.parametrize("curve", [0, 1])
def test_for_size_power_of_two_is_the_basic_domain(gpu, curve):
    m = 1 << 9
    v = gpu.synth_scalars(curve, 41, m)
    one, other = gpu.Domain(curve, m), gpu.Domain.for_size(curve, m)
    assert other.kind == gpu.Domain.BASIC and other.m == m and one.kind == gpu.Domain.BASIC
    for kind in range(4):
        assert np.array_equal(on_gpu(gpu, v, lambda p: one.fft(kind, p)), on_gpu(gpu, v, lambda p: other.fft(kind, p))), f"kind {kind}"
    one.close(); other.close()


def test_for_size_may_round_up(gpu):
    for curve, min_size, kind, m in ((0, 21, gpu.Domain.STEP, 24), (1, 21, gpu.Domain.STEP, 24), (0, 25, gpu.Domain.BASIC, 32),
                                     (0, 50000, gpu.Domain.BASIC, 1 << 16), (1, 50000, gpu.Domain.EXTENDED, 1 << 16),
                                     (1, (1 << 15) + (1 << 14) + 1, gpu.Domain.EXTENDED, 1 << 16)):
        dom = gpu.Domain.for_size(curve, min_size)
        assert (dom.kind, dom.m) == (kind, m), (curve, min_size)
        assert D.select(curve, min_size) == ({0: D.BASIC, 1: D.EXTENDED, 2: D.STEP}[kind], m)
        dom.close()


# what the reference's walk stops at and this library does not build: (curve, min_size, words the message must carry)
REFUSED = [(1, 5, ("mixed-radix", " 5 ")), (1, 10, ("mixed-radix", " 10 ")), (1, 25, ("mixed-radix", " 25 ")), (1, 40, ("mixed-radix", " 40 ")),
           (1, 5 << 15, ("mixed-radix", " 163840 ")),
           (1, (1 << 15) + (1 << 14), ("mixed-radix", " 51200 ", "candidate 7")), (1, 1 << 17, ("mixed-radix", " 163840 ", "candidate 7")),
           (1, (1 << 19) + (1 << 18), ("mixed-radix", " 819200 ", "candidate 7")),
           (1, 1 << 20, ("sequence domain", "1048576")),
           (0, 0, ("min_size",)), (0, 1, ("min_size",)), (1, 0, ("min_size",)), (1, 1, ("min_size",))]


@pytest.mark.parametrize("curve,min_size,needles", REFUSED)
def test_refused_sizes_name_the_reference_domain(gpu, curve, min_size, needles):
    assert D.select(curve, min_size)[0] in (D.MIXED, D.SEQUENCE, D.NONE)
    with pytest.raises(gpu.Mnt753Error) as e:
        gpu.Domain.for_size(curve, min_size)
    msg = str(e.value)
    assert "rc=-5" in msg, msg          # MNT753_EDOMAIN
    for needle in needles:
        assert needle in msg, msg
    if min_size > 1:
        assert str(min_size) in msg, msg


def test_domain_create_keeps_its_contract(gpu):
    """mnt753_domain_create is the basic radix-2 domain only: the sizes for_size accepts as step / extended are still refused there"""
    for curve, m in ((0, 24), (0, 3), (1, 1 << 16), (1, 96)):
        with pytest.raises(gpu.Mnt753Error):
            gpu.Domain(curve, m)
