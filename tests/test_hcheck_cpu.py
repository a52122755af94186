"""CPU: the spot check of compute_H, H(t) Z(t) = A(t) B(t) - C(t) at one point -- its model in Python integers (tests/hcheck_ref.py) on
every kind of domain, the accumulation and fold routines of csrc/reduce_kernels.hip.h compiled for the host with their limb bounds
asserted, and the new entry points of the C ABI without a device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import domain_ref as D
import golden_io as G
import hcheck_ref as H
import oracle_lib as O
from test_abi_cpu import exported, has_gpu, header_symbols

ROOT = O.ROOT
NEW = ["mnt753_vec_dot", "mnt753_poly_eval", "mnt753_domain_interp_at", "mnt753_h_check", "mnt753_compute_h_checked"]
DOMAINS = [(0, H.BASIC, 2), (0, H.BASIC, 8), (0, H.STEP, 3), (0, H.STEP, 24),
           (1, H.BASIC, 2), (1, H.BASIC, 8), (1, H.STEP, 3), (1, H.STEP, 24), (1, H.MIXED, 40)]
_CACHE = {}


def case(curve, kind, m):
    """satisfied random rows and their h, as integers; computed once per domain"""
    key = (curve, kind, m)
    if key not in _CACHE:
        ca, cb, cc = H.satisfied_rows(curve, m, 1000 * curve + 10 * m + len(kind))
        h_w = H.compute_h_wire(curve, kind, m, *(D.to_wire(curve, v) for v in (ca, cb, cc)))
        _CACHE[key] = (tuple(ca), tuple(cb), tuple(cc), tuple(D.from_wire(curve, h_w)))
    return _CACHE[key]


def points(curve, kind, m):
    """a random t, zero, and the last element of the domain"""
    dk = D.BASIC if kind == H.MIXED else kind
    return [H.random_t(curve, 77 + m), 0, D.elements(curve, dk, m)[-1]]


@pytest.mark.parametrize("curve,kind,m", DOMAINS)
def test_identity_holds_on_satisfied_rows(curve, kind, m):
    ca, cb, cc, h = case(curve, kind, m)
    assert h[m] == 0 and any(h)
    for t in points(curve, kind, m):
        lhs, rhs = H.sides(curve, kind, m, t, ca, cb, cc, h)
        assert lhs == rhs, (curve, kind, m, t)
    assert H.sides(curve, kind, m, points(curve, kind, m)[0], ca, cb, cc, h)[0] != 0      # not the trivial 0 == 0


@pytest.mark.parametrize("curve,kind,m", DOMAINS)
def test_identity_fails_after_one_change(curve, kind, m):
    ca, cb, cc, h = case(curve, kind, m)
    r = D.MODULUS[curve]
    t = points(curve, kind, m)[0]
    cc2 = list(cc)
    cc2[m // 2] = (cc2[m // 2] + 1) % r
    assert not H.holds(curve, kind, m, t, ca, cb, cc2, h)
    for idx in sorted({0, max(m - 2, 0), m - 1, m}):
        h2 = list(h)
        h2[idx] = (h2[idx] + 1) % r
        assert not H.holds(curve, kind, m, t, ca, cb, cc, h2), idx


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("logm", [3, 8])
def test_identity_fails_on_the_reference_h_of_unsatisfied_rows(curve, logm):
    """tests/golden/h_mnt{4,6}_{3,8}.bin: the reference's own h for random ca / cb / cc, whose rows are not satisfied"""
    m = 1 << logm
    ca, cb, cc, h = (D.from_wire(curve, x) for x in G.h(curve, logm))
    t = H.random_t(curve, 5 + logm)
    assert not H.holds(curve, H.BASIC, m, t, ca, cb, cc, h)
    # the same h is the quotient the check accepts once cc is what the rows demand: the remainder is what fails above
    r = D.MODULUS[curve]
    assert any(x * y % r != z for x, y, z in zip(ca, cb, cc))


def test_reduction_routines_compiled_for_the_host(tmp_path):
    """The accumulation, combine, Horner and finish routines the kernels call (csrc/reduce_kernels.hip.h are __host__ __device__) at
    all-(r - 1) operands over the longest per-thread sequence the launch geometry allows, the stated limb and value bounds asserted
    after every step, the results against plain fp_mul / fp_add."""
    exe = tmp_path / "host_dot_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tools", "host_dot_check.cpp")], check=True, timeout=600)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout + out.stderr


def test_new_entry_points_are_declared_exported_and_bound(pkg):
    declared = set(header_symbols())
    prod = exported(pkg.lib_path())
    L = pkg.lib()
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/mnt753_hip.h"
        assert name in prod, f"{name} is not exported by the product library"
        assert getattr(L, name).argtypes is not None, f"{name} is missing from the Python signature table"
    assert "mnt753_test_reduce_capped" in header_symbols("mnt753_hip_test.h")
    assert "mnt753_test_reduce_capped" in exported(pkg.api.test_lib_path())
    assert "mnt753_test_reduce_capped" not in prod
    assert ctypes.sizeof(pkg.HCheckResult) == 8 + 2 * 96
    for name in ("vec_dot", "poly_eval"):
        assert callable(getattr(pkg, name))
    for name in ("interp_at", "h_check", "compute_h_checked"):
        assert callable(getattr(pkg.Domain, name))


def test_bad_arguments_are_einval(pkg):
    L = pkg.lib()
    out = np.zeros(12, dtype=np.uint64)
    po = out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    t = H.wire1(0, 5)
    pt = t.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    big = np.full(12, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)                       # >= r
    r_w = D.ints_to_words([D.MODULUS[0]])[0].copy()                              # r itself
    dev = ctypes.c_void_p(8)
    assert L.mnt753_vec_dot(7, dev, dev, 1, po, None) == -1
    assert L.mnt753_vec_dot(0, None, dev, 1, po, None) == -1
    assert L.mnt753_vec_dot(0, dev, dev, 1, None, None) == -1
    assert L.mnt753_poly_eval(2, dev, 1, pt, po, None) == -1
    assert L.mnt753_poly_eval(0, None, 1, pt, po, None) == -1
    assert L.mnt753_poly_eval(0, dev, 1, None, po, None) == -1
    for bad_t in (big, r_w):
        assert L.mnt753_poly_eval(0, dev, 1, bad_t.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), po, None) == -1
        assert b"canonical" in L.mnt753_last_error()
    vecs = (ctypes.c_void_p * 3)(8, 8, 8)
    res = pkg.HCheckResult()
    assert L.mnt753_domain_interp_at(None, pt, vecs, 3, dev, po, None) == -1
    assert L.mnt753_h_check(None, pt, po, dev, ctypes.byref(res), None) == -1
    assert L.mnt753_compute_h_checked(None, dev, dev, dev, dev, pt, ctypes.byref(res), None) == -1
    assert not out.any() and res.ok == 0


@pytest.mark.skipif(has_gpu(), reason="checks the no-device behaviour")
def test_no_device_is_enodev(pkg):
    L = pkg.lib()
    out = np.zeros(12, dtype=np.uint64)
    po = out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    t = H.wire1(0, 5)
    dev = ctypes.c_void_p(8)
    assert L.mnt753_vec_dot(0, dev, dev, 1, po, None) == -2
    assert L.mnt753_vec_dot(0, None, None, 0, po, None) == -2
    assert L.mnt753_poly_eval(1, dev, 1, t.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), po, None) == -2
    with pytest.raises(pkg.Mnt753Error):
        pkg.vec_dot(0, 8, 8, 1)
    T = pkg.test_lib()
    assert T.mnt753_test_reduce_capped(0, 0, dev, dev, 1, None, 1, po) == -2


@pytest.mark.skipif(has_gpu(), reason="checks the no-device behaviour")
@pytest.mark.parametrize("how", ["flag", "env"])
def test_cli_check_h_fails_loudly_without_gpu(tmp_path, how):
    exe = os.path.join(ROOT, "snark-challenge-prover-reference_amd", "main_hip")
    params, inp, _ = G.e2e_paths(0)
    argv = [exe, "MNT4753", "compute", params, inp, str(tmp_path / "o.bin")]
    env = dict(os.environ)
    env.pop("MNT753_CHECK_H", None)
    if how == "flag":
        argv.append("--check-h")
    else:
        env["MNT753_CHECK_H"] = "1"
    r = subprocess.run(argv, capture_output=True, text=True, env=env)
    assert r.returncode == 1 and "no HIP device" in r.stderr, r.stderr
    assert not (tmp_path / "o.bin").exists()
    usage = subprocess.run([exe], capture_output=True, text=True)
    assert "--check-h" in usage.stdout + usage.stderr and "--check-h-t" in usage.stdout + usage.stderr
