"""CPU: the fixed-base batch scalar multiplication (mnt753_fixed_base_*, mnt753_batch_exp) as far as it goes without a device -- the
entry points exist and refuse to compute, the plan arithmetic the walk kernel shares with the host (csrc/batch_exp_plan.hpp) recodes
every structured scalar exactly and stays inside its table at every width, and the wrap family of tests/batch_exp_ref.py has the
digits it is built for."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import batch_exp_ref as BR
import msm_structured as S
import oracle_lib as O

ROOT = O.ROOT
WIDTHS = range(2, 23)   # every width mnt753_fixed_base_create accepts


def has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.mark.skipif(has_gpu(), reason="checks the no-device behaviour")
def test_create_refuses_without_a_device(pkg):
    """no CPU fallback: well-formed arguments, no device -> MNT753_ENODEV and a message"""
    L = pkg.lib()
    h = ctypes.c_void_p()
    point = np.ones(24, dtype=np.uint64)
    assert L.mnt753_fixed_base_create(0, 1, ctypes.c_void_p(point.ctypes.data), 4, 0, ctypes.byref(h)) == -2
    assert b"no HIP device" in L.mnt753_last_error()
    assert not h.value
    with pytest.raises(pkg.Mnt753Error):
        pkg.FixedBase(1, 2, np.ones(72, dtype=np.uint64))


def test_bad_arguments_come_before_the_device(pkg):
    """MNT753_EINVAL for what no device could make right, each with a message"""
    L = pkg.lib()
    h = ctypes.c_void_p()
    point = np.ones(72, dtype=np.uint64)
    p = ctypes.c_void_p(point.ctypes.data)
    for args in ((0, 1, p, 1, 0), (0, 1, p, 23, 0), (0, 1, p, -3, 0), (2, 1, p, 4, 0), (0, 3, p, 4, 0), (0, 1, None, 4, 0)):
        assert L.mnt753_fixed_base_create(*args, ctypes.byref(h)) == -1, args
        assert L.mnt753_last_error(), args
    assert L.mnt753_fixed_base_create(0, 1, p, 4, 0, None) == -1
    assert L.mnt753_batch_exp(None, p, 0, 1, None, p, 0, None) == -1
    assert L.mnt753_fixed_base_plan(None, (ctypes.c_int * 4)()) == -1
    assert L.mnt753_fixed_base_table_bytes(None) == 0 and L.mnt753_fixed_base_free(None) == 0


def all_scalars():
    ints = set()
    for curve in (0, 1):
        ints |= set(S.single_bits(curve)) | set(S.edges(curve)) | {0}
        ints |= {s for _, s in BR.wrap_family(curve)}
        for c in WIDTHS:
            ints |= set(S.extremes(curve, c)) | set(S.carry_chains(curve, c))
            if c <= 10:
                ints |= set(S.dense(curve, c))
    return sorted(ints)


@pytest.fixture(scope="module")
def scalar_file(tmp_path_factory):
    path = tmp_path_factory.mktemp("batch_exp") / "scalars.bin"
    ints = all_scalars()
    path.write_bytes(b"".join(v.to_bytes(96, "little") for v in ints))
    return str(path), len(ints)


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]],
                         ids=["plain", "asan_ubsan"])
def test_plan_arithmetic_compiled_for_the_host(tmp_path, scalar_file, flags):
    """tools/host_batch_exp_check.cpp over batch_exp_plan.hpp: at every width 2 .. 22 the digits of every structured and wrap scalar
    name rows inside the table, and the multiples |d| 2^(jw) those rows hold, signed, sum to the scalar.  Built plain and under
    ASan + UBSan; the program is run directly."""
    path, n = scalar_file
    exe = tmp_path / "host_batch_exp_check"
    subprocess.run(["g++", "-std=c++17", *flags, "-o", str(exe), os.path.join(ROOT, "tools", "host_batch_exp_check.cpp")], check=True, timeout=600)
    out = subprocess.run([str(exe), path], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and f"ALL OK: {n} scalars" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


@pytest.mark.parametrize("curve", [0, 1])
def test_wrap_family_has_its_digit_pattern(curve):
    """every member is below r, and wherever bit k is a window boundary the signed digits below it sum to -(r mod 2^k) and those above
    to floor(r / 2^k) 2^k: the two halves name the same point.  At the widths 5, 6, 7, 10, 11, 15, 17 and 22 one member has its k at the
    TOP window's boundary with one digit above it, inside the digit range."""
    r = BR.modulus(curve)
    fam = BR.wrap_family(curve)
    assert 1 <= len(fam) <= 53
    top_widths = set()
    for k, s in fam:
        assert 0 < s < r
        q, m = r >> k, r & ((1 << k) - 1)
        assert s == q * (1 << k) - m and ((q << k) + m) == r
        for c in WIDTHS:
            if k % c:
                continue
            d = S.booth(s, c)
            j = k // c
            assert S.unbooth(d, c) == s
            assert S.unbooth(d[:j], c) == -m, (k, c)
            assert sum(x << ((j + i) * c) for i, x in enumerate(d[j:])) == q << k, (k, c)
            if j == S.windows(c) - 1:
                assert d[-1] == q and 0 < q <= 1 << (c - 1)
                top_widths.add(c)
    assert top_widths >= {5, 6, 7, 10, 11, 15, 17, 22}, sorted(top_widths)
