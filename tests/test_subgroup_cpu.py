"""CPU: the subgroup test of G2 as far as it goes without a device.

* tests/subgroup_ref.py -- psi(P) == [t - 1] P in Python integers -- against the definition [r] P == O on the generator, a multiple
  of it, three lifted twist points per curve, their cofactor parts [r] P and Q + [r] P with Q in G2.  The GPU tests stand on it.
* tools/host_subgroup_check.cpp: the device's own source (Ate<C>::endo / step_loop / run_equals / affine_equals) through the one-lane
  fields under g++, on points written here, with a running point of Z = 0 and an all-zero one, which must be refused.
* the ABI: symbols declared, exported and in the sanitizer stub; the Python names; argument errors without a device; the CLI's usage
  errors; `check --subgroup` and `verify --check-subgroup` through the `make asan` stub binary (a stand-alone program)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import subgroup_ref as S
from test_abi_cpu import exported, has_gpu, header_symbols
from test_validate_cpu import EXE, NAME, asan, g16, run_san  # noqa: F401  (asan: the module-scoped fixture that runs `make asan`)

ROOT = O.ROOT
NEW = ("mnt753_check_subgroup", "mnt753_groth16_verify_ex")
HOOKS = ("mnt753_test_g2_endomorphism", "mnt753_test_g2_loop_multiple")


@pytest.mark.parametrize("curve", [0, 1])
def test_reference_agrees_with_the_definition(curve):
    C = S.CURVES[curve]
    G = C.gen(2)
    members = [G, S.generator_multiple(curve, 0xC0FFEE), C.neg(G), None]
    for pt in members:
        assert S.in_subgroup_by_definition(curve, pt) and S.in_subgroup(curve, pt)
    off = S.off_subgroup_points(curve)
    assert [len(v) for v in off.values()] == [3, 3, 3]
    for kind, pts in off.items():
        for pt in pts:
            assert pt is not None and C.on_curve(pt, 2), kind
            assert not S.in_subgroup_by_definition(curve, pt), kind      # [r] P != O: really outside G2
            assert not S.in_subgroup(curve, pt), kind
    # psi is an endomorphism of the twist with psi^2 - t psi + q = 0, on members and on the others
    t = C.q + 1 - C.r
    for pt in (G, off["lifted"][0], off["mixed"][1]):
        p1 = S.psi(curve, pt)
        assert C.on_curve(p1, 2)
        lhs = C.add(S.psi(curve, p1), C.mul(C.q, pt, 2), 2)
        assert lhs == S.signed_mul(curve, t, p1)
    assert S.psi(curve, C.add(G, off["lifted"][0], 2)) == C.add(S.psi(curve, G), S.psi(curve, off["lifted"][0]), 2)
    assert S.loop_multiplier(curve) == t - 1 and (S.loop_multiplier(curve) - C.q) % C.r == 0


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("host_subgroup") / "host_subgroup_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tools", "host_subgroup_check.cpp")], check=True, timeout=600)
    return str(exe)


@pytest.mark.parametrize("curve", [0, 1])
def test_device_source_on_the_host(host_check, curve, tmp_path):
    C = S.CURVES[curve]
    off = S.off_subgroup_points(curve)
    pts = [(C.gen(2), 1), (S.generator_multiple(curve, 12345), 1), (C.neg(C.gen(2)), 1)]
    pts += [(off[kind][i], 0) for kind, i in (("lifted", 0), ("lifted", 1), ("cofactor", 0), ("mixed", 0), ("mixed", 2))]
    rec = [np.array([curve, len(pts)], dtype=np.uint64)]
    for pt, member in pts:
        rec += [S.words(curve, pt), S.words(curve, S.psi(curve, pt)), np.array([member], dtype=np.uint64)]
    path = tmp_path / "points.bin"
    np.concatenate(rec).astype("<u8").tofile(path)
    r = subprocess.run([host_check, str(path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout + r.stderr
    assert "Z = 0: 0 0, all-zero R: 0 0" in r.stdout, r.stdout
    # the program does fail where a verdict is wrong: the first member marked as outside
    flipped = np.concatenate(rec).astype("<u8")
    flipped[2 + 2 * 24 * C.deg] = 0
    flipped.tofile(path)
    r = subprocess.run([host_check, str(path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "FAILURES" in r.stdout


def test_symbols_are_declared_exported_and_stubbed(pkg):
    syms = header_symbols()
    L = ctypes.CDLL(pkg.lib_path())
    for s in NEW:
        assert s in syms, f"{s} not declared in include/mnt753_hip.h"
        assert hasattr(L, s), f"{s} not exported"
    assert set(NEW) <= exported(pkg.lib_path())
    assert set(HOOKS) <= set(header_symbols("mnt753_hip_test.h")) and set(HOOKS) <= exported(pkg.api.test_lib_path())
    text = open(os.path.join(ROOT, "include", "mnt753_hip.h")).read()
    assert "MNT753_BAD_NOT_IN_SUBGROUP = 4" in text and "#define MNT753_VERIFY_CHECK_SUBGROUP 1u" in text
    stub = open(os.path.join(ROOT, "tools", "stub_abi", "stub_mnt753.cpp")).read()
    for s in NEW:
        assert f"int {s}(" in stub
    assert pkg.BAD_NOT_IN_SUBGROUP == 4 and pkg.VERIFY_CHECK_SUBGROUP == 1
    assert callable(pkg.check_subgroup) and callable(pkg.VerificationKey.check_subgroup)
    import inspect
    assert inspect.signature(pkg.VerificationKey.verify).parameters["check_subgroup"].default is False
    assert list(inspect.signature(pkg.check_subgroup).parameters) == ["curve", "group", "affine", "on_device", "n", "stream"]
    assert callable(pkg.api.test_g2_endomorphism) and callable(pkg.api.test_g2_loop_multiple)


def test_argument_errors_without_a_device(pkg):
    L = pkg.lib()
    rep = pkg.CheckReport()
    buf = np.zeros(72, dtype=np.uint64)
    p = ctypes.c_void_p(buf.ctypes.data)
    EINVAL = -1
    assert L.mnt753_check_subgroup(2, 2, p, 0, 1, ctypes.byref(rep), None) == EINVAL
    assert L.mnt753_check_subgroup(0, 3, p, 0, 1, ctypes.byref(rep), None) == EINVAL
    assert L.mnt753_check_subgroup(0, 2, None, 0, 1, ctypes.byref(rep), None) == EINVAL
    assert L.mnt753_check_subgroup(1, 2, p, 0, 1, None, None) == EINVAL
    assert L.mnt753_check_subgroup(1, 1, None, 0, 1, ctypes.byref(rep), None) == EINVAL
    assert b"check_subgroup" in L.mnt753_last_error()
    # an unknown flag bit is refused before anything else is looked at (a key cannot exist without a device: any non-null handle)
    v = np.zeros(1, dtype=np.uint8)
    assert L.mnt753_groth16_verify_ex(p, p, p, 1, 0, 2, ctypes.c_void_p(v.ctypes.data), None) == EINVAL
    assert L.mnt753_groth16_verify_ex(p, p, p, 1, 0, 0x80000001, ctypes.c_void_p(v.ctypes.data), None) == EINVAL
    assert L.mnt753_groth16_verify_ex(None, p, p, 1, 0, 1, ctypes.c_void_p(v.ctypes.data), None) == EINVAL
    TL = pkg.api.test_lib()
    q = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    assert TL.mnt753_test_g2_endomorphism(2, q, 1, q) == EINVAL and TL.mnt753_test_g2_loop_multiple(0, None, 1, q) == EINVAL


@pytest.mark.skipif(has_gpu(), reason="checks the no-device behaviour")
def test_refuses_without_a_device(pkg):
    L = pkg.lib()
    rep = pkg.CheckReport()
    buf = np.zeros(72, dtype=np.uint64)
    p = ctypes.c_void_p(buf.ctypes.data)
    for n in (0, 1):
        assert L.mnt753_check_subgroup(0, 2, p, 0, n, ctypes.byref(rep), None) == -2
        assert L.mnt753_check_subgroup(1, 1, p, 0, n, ctypes.byref(rep), None) == -2
    with pytest.raises(pkg.Mnt753Error):
        pkg.check_subgroup(1, 2, buf)


def test_cli_usage():
    params = g16(0, "params.bin")
    for args in (["MNT4753", "check", "--subgroup"], ["MNT4753", "check", params, "--subgroups"], ["MNT4753", "check-r1cs", params, params, params, "--subgroup"],
                 ["MNT4753", "verify", params, params, "--check-subgroup"], ["MNT4753", "verify", params, params, params, "--check-subgroups"],
                 ["MNT4753", "vk", params, "/dev/null", "--check-subgroup"]):
        r = subprocess.run([EXE] + args, capture_output=True, text=True)
        assert r.returncode == 2, (args, r.returncode, r.stderr)
    r = subprocess.run([EXE, "MNT4753", "check"], capture_output=True, text=True)
    assert "--subgroup" in r.stderr
    r = subprocess.run([EXE, "MNT4753", "verify"], capture_output=True, text=True)
    assert "--check-subgroup" in r.stderr


def elements_file(curve, tmp_path):
    """alpha_g1 | beta_g2 | delta_g2 | ABC_g1 of the right sizes for one public input (the stub does no arithmetic)"""
    w2 = 24 * (2 if curve == 0 else 3)
    path = tmp_path / "vk_elements.bin"
    np.arange(1, 24 + 2 * w2 + 48 + 1, dtype="<u8").tofile(path)
    return str(path)


@pytest.mark.parametrize("curve", [0, 1])
def test_cli_over_the_stub_under_asan(asan, curve, tmp_path):
    params, inp = g16(curve, "params.bin"), g16(curve, "input.bin")
    r = run_san(asan, [NAME[curve], "check", params, "--subgroup"], 0)
    assert "B2:" in r.stdout and "points ok" in r.stdout
    r = run_san(asan, [NAME[curve], "check", params, inp, "--subgroup"], 3, {"MNT753_STUB_BAD_SUBGROUP": "3"})
    assert "B2: 1 bad, first at 3: not in the subgroup" in r.stdout and "A: " in r.stdout and "bad" not in r.stdout.split("B2:")[0]
    # the knob touches nothing without the option; with several devices the index is the file's
    run_san(asan, [NAME[curve], "check", params], 0, {"MNT753_STUB_BAD_SUBGROUP": "3"})
    r = run_san(asan, [NAME[curve], "check", params, "--subgroup", "--gpus", "2"], 3, {"MNT753_STUB_BAD_SUBGROUP": "1"})
    assert "B2: 2 bad, first at 1: not in the subgroup" in r.stdout
    # an earlier reason wins over the subgroup test
    r = run_san(asan, [NAME[curve], "check", params, "--subgroup"], 3, {"MNT753_STUB_BAD_SUBGROUP": "3", "MNT753_STUB_BAD_POINT": "5"})
    assert "B2: 1 bad, first at 5: off curve" in r.stdout
    el, proof = elements_file(curve, tmp_path), g16(curve, "full.bin")
    r = run_san(asan, [NAME[curve], "verify", el, inp, proof, proof, "--check-subgroup"], 0)
    assert r.stdout.split() == ["VERIFIED", "VERIFIED"]
    r = run_san(asan, [NAME[curve], "verify", el, inp, proof, proof, "--check-subgroup"], 3, {"MNT753_STUB_BAD_B": "1"})
    assert r.stdout.splitlines() == ["VERIFIED", "REJECTED (B not in the subgroup)"]
    r = run_san(asan, [NAME[curve], "verify", el, inp, proof, proof], 0, {"MNT753_STUB_BAD_B": "1"})
    assert r.stdout.split() == ["VERIFIED", "VERIFIED"]
    r = run_san(asan, [NAME[curve], "verify", el, inp, proof, "--check-subgroup"], 3, {"MNT753_STUB_BAD_SUBGROUP": "1"})
    assert "delta_g2 of the key: not in the subgroup" in r.stderr and r.stdout == ""
    r = run_san(asan, [NAME[curve], "verify", el, inp, proof, "--check-subgroup"], 3, {"MNT753_STUB_BAD_SUBGROUP": "0"})
    assert "beta_g2 of the key: not in the subgroup" in r.stderr and r.stdout == ""
