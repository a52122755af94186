"""GPU: the mixed-radix evaluation domains of MNT6753 (m = 2^a 5^b, kind MNT753_DOMAIN_MIXED), bit-exact.

* selection: Domain.for_size(1, n, mixed=True) builds what tests/domain_ref.select says the reference builds; without the flag,
  on MNT4753 and past candidate 7 nothing changes; Domain.mixed is the exact-size constructor;
* transforms: all four kinds and divide_by_Z_on_coset against the DEFINITION (the polynomial's values at omega^k, domain_ref with
  kind BASIC) up to m = 200 and against tests/mixed_domain_ref.py's fast composition above (pinned to the definition by
  tests/test_mixed_domains_cpu.py), at the sizes where each piece of the schedule can go wrong;
* structured inputs at the two full sizes 5 * 2^15 and 25 * 2^15, where the expected transform has a closed form;
* compute_H against the model, equal to its split form, and on a domain that lives on logical device 1."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import domain_ref as D
import mixed_domain_ref as MX

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOD = D.MODULUS[1]
RM = D.R % MOD                      # the Montgomery form of 1

# T = 1 (no inner transform) | T = 2 | T = 8: merge widths 8 and 40, below 64 and no multiple of it | T = 64: exactly one block
# column | T = 2^9: the inner transform takes two k_ntt_group passes through the inner work buffer
SIZES = [5, 25, 10, 50, 40, 200, 320, 1600, 5 << 9, 25 << 9]
FULL = [5 << 15, 25 << 15]


def words(ints):
    return D.ints_to_words(ints)


def on_gpu(gpu, vec, *fns):
    """fn(device pointer), one after the other, on a device copy of the wire array vec -> the array afterwards"""
    buf = gpu.DeviceBuffer.from_numpy(np.ascontiguousarray(vec, dtype=np.uint64))
    for fn in fns:
        fn(buf.ptr.value)
    out = buf.to_numpy().reshape(-1, 12)
    buf.close()
    return out


# ---- selection ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(5, 5), (10, 10), (25, 25), (40, 40), (5 << 15, 5 << 15), ((1 << 15) + (1 << 14), 51200), (1 << 17, 163840),
                                 ((1 << 19) + (1 << 18), 819200)])
def test_for_size_with_the_flag_builds_the_mixed_domain(gpu, n, m):
    assert D.select(1, n) == (D.MIXED, m)
    dom = gpu.Domain.for_size(1, n, mixed=True)
    assert (dom.kind, dom.m) == (gpu.Domain.MIXED, m) and gpu.Domain.MIXED == 3
    dom.close()
    with pytest.raises(gpu.Mnt753Error) as e:            # and without it the refusal stands
        gpu.Domain.for_size(1, n)
    assert "mixed-radix" in str(e.value) and "rc=-5" in str(e.value)


def test_what_stays_refused_with_the_flag(gpu):
    with pytest.raises(gpu.Mnt753Error) as e:
        gpu.Domain.for_size(1, 819201, mixed=True)
    assert "rc=-5" in str(e.value) and "sequence domain" in str(e.value) and "819201" in str(e.value)
    for n in (0, 1):
        with pytest.raises(gpu.Mnt753Error) as e:
            gpu.Domain.for_size(1, n, mixed=True)
        assert "min_size" in str(e.value)


def test_the_flag_changes_nothing_else(gpu):
    dom = gpu.Domain.for_size(0, 40, mixed=True)         # MNT4753 has no small subgroup: the step domain of 40, as without the flag
    assert (dom.kind, dom.m) == (gpu.Domain.STEP, 40) and D.select(0, 40) == (D.STEP, 40)
    dom.close()
    for n, kind, m in ((96, gpu.Domain.STEP, 96), (1 << 9, gpu.Domain.BASIC, 1 << 9), (50000, gpu.Domain.EXTENDED, 1 << 16)):
        dom = gpu.Domain.for_size(1, n, mixed=True)
        assert (dom.kind, dom.m) == (kind, m)
        dom.close()


def test_the_exact_constructor(gpu):
    for m in (64, 125, 3 * 5, 5 << 16, 0, 1):
        assert not MX.is_mixed_size(m)
        with pytest.raises(gpu.Mnt753Error) as e:
            gpu.Domain.mixed(1, m)
        assert "rc=-5" in str(e.value)
    for m in (5, 40, 64, 5 << 15):                       # every size on MNT4753
        with pytest.raises(gpu.Mnt753Error) as e:
            gpu.Domain.mixed(0, m)
        assert "rc=-5" in str(e.value)
    for m in (5, 40):                                    # the powers of two stay with Domain(curve, m), the mixed sizes are not its
        with pytest.raises(gpu.Mnt753Error):
            gpu.Domain(1, m)
        dom = gpu.Domain.mixed(1, m)
        assert (dom.kind, dom.m) == (gpu.Domain.MIXED, m)
        dom.close()


# ---- transforms against the model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", SIZES)
def test_transforms_against_the_model(gpu, m):
    assert MX.is_mixed_size(m)
    rng = random.Random(0x6d6978 + m)
    v = [rng.randrange(MOD) for _ in range(m)]           # seeded uniform (the transforms are linear: these are the Montgomery integers)
    if m <= 200:
        fft = {c: D.fft_def(1, D.BASIC, m, v, c) for c in (False, True)}
    else:
        fft = {c: MX.fast_fft(m, v, c) for c in (False, True)}
    ifft = {c: MX.fast_ifft(m, v, c) for c in (False, True)}
    if m <= 200:                                         # an inverse by definition: its forward transform is the input
        assert all(D.is_ifft_of(1, D.BASIC, m, ifft[c], v, c) for c in (False, True))
    dom = gpu.Domain.mixed(1, m)
    w = words(v)
    assert np.array_equal(on_gpu(gpu, w, lambda p: dom.fft(gpu.FFT, p)), words(fft[False])), "FFT"
    assert np.array_equal(on_gpu(gpu, w, lambda p: dom.fft(gpu.COSET_FFT, p)), words(fft[True])), "cosetFFT"
    assert np.array_equal(on_gpu(gpu, w, lambda p: dom.fft(gpu.IFFT, p)), words(ifft[False])), "iFFT"
    assert np.array_equal(on_gpu(gpu, w, lambda p: dom.fft(gpu.ICOSET_FFT, p)), words(ifft[True])), "icosetFFT"
    # the inverses, additionally, on the device alone
    assert np.array_equal(on_gpu(gpu, w, lambda p: dom.fft(gpu.IFFT, p), lambda p: dom.fft(gpu.FFT, p)), w), "FFT(iFFT(v))"
    assert np.array_equal(on_gpu(gpu, w, lambda p: dom.fft(gpu.ICOSET_FFT, p), lambda p: dom.fft(gpu.COSET_FFT, p)), w), "cosetFFT(icosetFFT(v))"
    # divide_by_Z_on_coset: Z(g x) = g^m - 1 at every element
    zi = MX.z_inverse(m)
    assert zi * D.vanishing(1, D.BASIC, m, D.G * D.element(1, D.BASIC, m, m - 1) % MOD) % MOD == 1
    assert np.array_equal(on_gpu(gpu, w, lambda p: dom.divide_by_z_on_coset(p)), words([x * zi % MOD for x in v])), "divide_by_Z_on_coset"
    dom.close()


# ---- structured inputs at full size --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full_domains(gpu):
    doms = {m: gpu.Domain.mixed(1, m) for m in FULL}
    yield doms
    for d in doms.values():
        d.close()


def running(first, ratio, n):
    """first * ratio^k for k < n, as one wire array"""
    return D.ints_to_words(D._powers(ratio, n, MOD, first))


@pytest.mark.parametrize("kind", ["FFT", "IFFT", "COSET_FFT", "ICOSET_FFT"])
@pytest.mark.parametrize("which", ["1", "Q", "T", "m-1"])
@pytest.mark.parametrize("m", FULL)
def test_unit_vectors_at_full_size(gpu, full_domains, m, which, kind):
    """FFT(e_j)[k] = omega^(j k) for every k, by a running product; cosetFFT: g^j omega^(j k); iFFT: omega^(-j k) / m;
    icosetFFT: g^-k omega^(-j k) / m"""
    q, t = MX.split(m)
    j = {"1": 1, "Q": q, "T": t, "m-1": m - 1}[which]
    w = D.root_of_unity(1, m)
    wj, ginv, minv = pow(w, j, MOD), pow(D.G, -1, MOD), pow(m, -1, MOD)
    wj_inv = pow(wj, -1, MOD)
    first, ratio = {"FFT": (RM, wj), "COSET_FFT": (RM * pow(D.G, j, MOD), wj), "IFFT": (RM * minv, wj_inv),
                    "ICOSET_FFT": (RM * minv, wj_inv * ginv % MOD)}[kind]
    e = np.zeros((m, 12), dtype=np.uint64)
    e[j] = words([RM])[0]
    got = on_gpu(gpu, e, lambda p: full_domains[m].fft(getattr(gpu, kind), p))
    assert np.array_equal(got, running(first, ratio, m))


@pytest.mark.parametrize("m", FULL)
def test_constant_vector_at_full_size(gpu, full_domains, m):
    c = 0x1234567 * RM % MOD
    got = on_gpu(gpu, np.tile(words([c]), (m, 1)), lambda p: full_domains[m].fft(gpu.FFT, p))
    want = np.zeros((m, 12), dtype=np.uint64)
    want[0] = words([c * m % MOD])[0]
    assert np.array_equal(got, want)


@pytest.mark.parametrize("m", FULL)
def test_uniform_vector_at_full_size(gpu, full_domains, m):
    dom = full_domains[m]
    x = gpu.synth_scalars(1, 0x756e69 + m, m).reshape(m, 12)
    f = on_gpu(gpu, x, lambda p: dom.fft(gpu.FFT, p))
    assert np.array_equal(on_gpu(gpu, f, lambda p: dom.fft(gpu.IFFT, p)), x), "iFFT(FFT(x))"
    assert np.array_equal(on_gpu(gpu, x, lambda p: dom.fft(gpu.COSET_FFT, p), lambda p: dom.fft(gpu.ICOSET_FFT, p)), x), "icosetFFT(cosetFFT(x))"
    xi, fi = D.mont_ints(x), D.mont_ints(f)
    rng = random.Random(m)
    for k in [0, m - 1] + rng.sample(range(1, m - 1), 2):      # FFT(x)[k] by Horner at omega^k
        assert fi[k] == D.fft_at(1, D.BASIC, m, xi, k), k


# ---- compute_H ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [40, 200, 5 << 9, 25 << 9])
def test_compute_h_against_the_model_and_its_split_form(gpu, m):
    ca, cb, cc = (gpu.synth_scalars(1, 800 + i, m).reshape(m, 12) for i in range(3))
    want = MX.fast_compute_h_steps(m, ca, cb, cc)
    dom = gpu.Domain.for_size(1, m, mixed=True)
    assert dom.kind == gpu.Domain.MIXED
    a, b, c = (gpu.DeviceBuffer.from_numpy(x) for x in (ca, cb, cc))
    dh = gpu.DeviceBuffer(96 * (m + 1))
    dom.compute_h(a.ptr.value, b.ptr.value, c.ptr.value, dh.ptr.value)
    h = dh.to_numpy().reshape(m + 1, 12)
    assert np.array_equal(h, words(want["h"] + [0])), "compute_h"
    # compute_h == three _chain + one _finish
    a2, b2, c2 = (gpu.DeviceBuffer.from_numpy(x) for x in (ca, cb, cc))
    for v in (a2, b2, c2):
        dom.compute_h_chain(v.ptr.value)
    assert np.array_equal(b2.to_numpy().reshape(m, 12), words(want["cos"][1])), "compute_h_chain"
    dh2 = gpu.DeviceBuffer(96 * (m + 1))
    dom.compute_h_finish(a2.ptr.value, b2.ptr.value, c2.ptr.value, dh2.ptr.value)
    assert np.array_equal(dh2.to_numpy().reshape(m + 1, 12), h), "compute_h_chain x3 + compute_h_finish"
    for x in (a, b, c, dh, a2, b2, c2, dh2):
        x.close()
    dom.close()


ON_DEVICE_1 = r'''
import json, sys
sys.path.insert(0, %(root)r)
import ctypes as C
import numpy as np
from __graft_entry__ import load_package
pkg = load_package()
L = pkg.api.lib()
assert L.mnt753_init_devices(2) == 0, L.mnt753_last_error().decode()
m = %(m)d
vecs = [pkg.synth_scalars(1, 800 + i, m) for i in range(3)]
out = {}
for dev in (0, 1):
    assert L.mnt753_set_device(dev) == 0
    dom = pkg.Domain.mixed(1, m)                     # lives on the device that is current now
    out["device%%d" %% dev] = int(L.mnt753_domain_device(dom._h))
    bufs = [pkg.DeviceBuffer.from_numpy(x) for x in vecs]
    dh = pkg.DeviceBuffer(96 * (m + 1))
    assert L.mnt753_set_device(0) == 0               # the calls run on the domain's device whatever the current one is
    dom.compute_h(bufs[0].ptr.value, bufs[1].ptr.value, bufs[2].ptr.value, dh.ptr.value)
    L.mnt753_set_device(dev)
    out["h%%d" %% dev] = dh.to_numpy().tobytes().hex()
    v = pkg.DeviceBuffer.from_numpy(vecs[0])
    dom.fft(pkg.FFT, v.ptr.value)
    out["fft%%d" %% dev] = v.to_numpy().tobytes().hex()
    L.mnt753_domain_free(dom._h); dom._h = C.c_void_p()
print(json.dumps(out), flush=True)
'''


def test_a_mixed_domain_on_logical_device_1(gpu):
    """Under MNT753_SHARE_DEVICE=1 two logical devices map onto the one GPU: a mixed domain created while device 1 is current lives
    there, and compute_H and the FFT on it give the model's words.  A fresh child process: the devices are set up once per process."""
    m = 200
    r = subprocess.run([sys.executable, "-c", ON_DEVICE_1 % {"root": ROOT, "m": m}], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, MNT753_SHARE_DEVICE="1"))
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert (out["device0"], out["device1"]) == (0, 1)
    ca, cb, cc = (gpu.synth_scalars(1, 800 + i, m).reshape(m, 12) for i in range(3))
    want_h = MX.fast_compute_h(m, ca, cb, cc).tobytes().hex()
    want_f = words(D.fft_def(1, D.BASIC, m, D.mont_ints(ca))).tobytes().hex()
    for dev in (0, 1):
        assert out["h%d" % dev] == want_h and out["fft%d" % dev] == want_f, dev
