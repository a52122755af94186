"""CPU: the mixed-radix evaluation domains of MNT6753 (m = 2^a 5^b) without a GPU.

* tests/mixed_domain_ref.py's fast composition -- what the GPU tests compare whole vectors with above m = 200 -- equals the
  definition (tests/domain_ref.py with kind BASIC: the polynomial's values at omega^k, omega = libff's get_root_of_unity(m));
* the library exports the new entry points and, without a device, answers MNT753_ENODEV from them;
* `main_hip --mixed-radix` and MNT753_MIXED_RADIX=1 are parsed by compute and complete, against the stub of the C ABI."""
import ctypes
import os
import random
import subprocess

import pytest

import domain_ref as D
import golden_io as G
import mixed_domain_ref as MX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [5, 10, 25, 40, 50, 200]


@pytest.mark.parametrize("m", SIZES)
def test_fast_composition_equals_the_definition(m):
    r = D.MODULUS[1]
    rng = random.Random(5000 + m)
    v = [rng.randrange(r) for _ in range(m)]
    w = D.root_of_unity(1, m)
    assert pow(w, m, r) == 1 and all(pow(w, m // p, r) != 1 for p in (2, 5) if m % p == 0)       # a primitive m-th root
    xs = D.elements(1, D.BASIC, m)
    assert len(set(xs)) == m and all(D.vanishing(1, D.BASIC, m, x) == 0 for x in xs)
    for coset in (False, True):
        f = D.fft_def(1, D.BASIC, m, v, coset)
        assert MX.fast_fft(m, v, coset) == f
        assert MX.fast_ifft(m, f, coset) == v
        assert D.is_ifft_of(1, D.BASIC, m, MX.fast_ifft(m, v, coset), v, coset)
    assert [p * MX.z_inverse(m) % r for p in v] == D.divide_by_z_on_coset_def(1, D.BASIC, m, v)


@pytest.mark.parametrize("m", [10, 50])
def test_compute_h_composition_satisfies_the_definition(m):
    """H(x) Z(x) = A(x) B(x) - C(x) on the coset, A, B, C the interpolants of ca, cb, cc on the domain"""
    r = D.MODULUS[1]
    rng = random.Random(11 * m)
    plain = [[rng.randrange(r) for _ in range(m)] for _ in range(3)]
    h = D.from_wire(1, MX.fast_compute_h(m, *(D.to_wire(1, v) for v in plain)))
    assert h[m] == 0
    A, B, C = (MX.fast_ifft(m, v) for v in plain)
    for x in D.elements(1, D.BASIC, m):
        t = D.G * x % r
        assert D._horner(h[:m], t, r) * D.vanishing(1, D.BASIC, m, t) % r == (D._horner(A, t, r) * D._horner(B, t, r) - D._horner(C, t, r)) % r


def test_sizes_the_exact_constructor_accepts():
    ok = [m for m in range(1, 2000) if MX.is_mixed_size(m)]
    assert ok == sorted(q << a for q in (5, 25) for a in range(16) if (q << a) < 2000)
    assert MX.is_mixed_size(25 << 15) and not MX.is_mixed_size(5 << 16) and not MX.is_mixed_size(125) and not MX.is_mixed_size(64)
    assert all(D.select(1, m) == (D.MIXED, m) for m in ok)


def test_the_library_exports_the_new_entry_points(pkg):
    L = ctypes.CDLL(pkg.lib_path())
    for name in ("mnt753_domain_create_mixed", "mnt753_domain_create_for_ex"):
        assert hasattr(L, name), name
    assert pkg.Domain.MIXED == MX.KIND_CODE == 3 and pkg.Domain.ALLOW_MIXED == 1
    header = open(os.path.join(ROOT, "include", "mnt753_hip.h")).read()
    assert "#define MNT753_DOMAIN_MIXED 3" in header and "#define MNT753_DOMAIN_ALLOW_MIXED 1u" in header


def test_create_mixed_without_a_device(pkg):
    """no silent fallback: the new constructors answer MNT753_ENODEV before a device is initialised, like their siblings"""
    try:
        import torch
        if torch.cuda.is_available():
            pytest.skip("a GPU is present: the library initialises")
    except ImportError:
        pass
    L = ctypes.CDLL(pkg.lib_path())
    L.mnt753_domain_create_mixed.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p)]
    L.mnt753_domain_create_for_ex.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.c_uint, ctypes.POINTER(ctypes.c_void_p)]
    h = ctypes.c_void_p()
    for m in (5, 40, 25 << 15):
        assert L.mnt753_domain_create_mixed(1, m, ctypes.byref(h)) == -2       # MNT753_ENODEV
        assert L.mnt753_domain_create_for_ex(1, m, 1, ctypes.byref(h)) == -2
    assert L.mnt753_domain_create_for_ex(1, 40, 0, ctypes.byref(h)) == -2
    assert L.mnt753_domain_create_for_ex(1, 40, 2, ctypes.byref(h)) == -1      # an unknown flag bit: MNT753_EINVAL
    assert L.mnt753_domain_create_mixed(1, 40, None) == -1


@pytest.fixture(scope="module")
def asan_exe():
    r = subprocess.run(["make", "asan"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return os.path.join(ROOT, "build", "san", "main_hip_asan")


def test_main_hip_parses_mixed_radix_against_the_stub(asan_exe, tmp_path):
    params, inp, _ = G.e2e_paths(1)
    out = str(tmp_path / "o")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for flags, extra in ((["--mixed-radix"], {}), (["--mixed-radix", "--repeat", "2", "--gpus", "2"], {}), (["--validate", "--mixed-radix"], {}),
                         ([], {"MNT753_MIXED_RADIX": "1"}), ([], {"MNT753_MIXED_RADIX": "0"})):
        r = subprocess.run([asan_exe, "MNT6753", "compute", params, inp, out] + flags, capture_output=True, text=True, env=dict(env, **extra), timeout=600)
        assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
        assert "Total time from input to output" in r.stdout
    # an option the prover does not have is still refused, next to the new one
    r = subprocess.run([asan_exe, "MNT6753", "compute", params, inp, out, "--mixed-radix", "--mixed"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 2 and "unknown option --mixed" in r.stderr
    # complete: the option is taken where --validate is (a missing key file is the I/O failure it was, not a usage error)
    r = subprocess.run([asan_exe, "MNT6753", "complete", "/nonexistent", inp, inp, out, "--mixed-radix"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 1 and "Sanitizer" not in r.stderr, r.stderr[-2000:]
