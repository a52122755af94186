"""CPU: input validation (include/mnt753_hip.h "input validation", csrc/mnt753_validate.hip) as far as it goes without a device:
the ABI is there and refuses to compute without a GPU, the CLI modes parse, the host paths are clean under the sanitizers over the
test stub -- and the big-integer model the GPU tests compare the device with (tests/validate_ref.py) calls every fixture the
REFERENCE wrote well formed: that is the ground the GPU tests stand on ("good inputs give n_bad = 0")."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import golden_io as G
import oracle_lib as O
import validate_ref as V
from test_abi_cpu import exported, has_gpu, header_symbols

ROOT = O.ROOT
EXE = os.path.join(ROOT, "snark-challenge-prover-reference_amd", "main_hip")
NAME = {0: "MNT4753", 1: "MNT6753"}
CHECKS = ("mnt753_check_points", "mnt753_check_scalars", "mnt753_check_products", "mnt753_r1cs_check")


def g16(curve, name):
    return os.path.join(G.GOLDEN, f"g16_mnt{4 if curve == 0 else 6}", name)


# (curve, params, input) of every parameter file the reference's generator wrote (oracle/mint_golden.cpp:238-239, 274-277,
# oracle/ref_groth16.cpp:55-78)
FIXTURES = [(0,) + G.e2e_paths(0)[:2], (1,) + G.e2e_paths(1)[:2], (1,) + G.e2e_fast_mnt6_paths()[:2],
            (0, g16(0, "params.bin"), g16(0, "input.bin")), (1, g16(1, "params.bin"), g16(1, "input.bin"))]
FIXTURE_IDS = ["e2e_mnt4", "e2e_mnt6", "e2e_mnt6_2p10", "g16_mnt4", "g16_mnt6"]


def test_check_symbols_are_declared_and_exported(pkg):
    syms = header_symbols()
    L = ctypes.CDLL(pkg.lib_path())
    for s in CHECKS:
        assert s in syms, f"{s} not declared in include/mnt753_hip.h"
        assert hasattr(L, s), f"{s} not exported"
    assert set(CHECKS) <= exported(pkg.lib_path())
    for name in ("check_points", "check_scalars", "check_products", "CheckReport", "BAD_NONCANONICAL", "BAD_OFF_CURVE", "BAD_UNSATISFIED"):
        assert hasattr(pkg, name)
    assert hasattr(pkg.R1cs, "check")
    assert ctypes.sizeof(pkg.CheckReport) == 24
    text = open(os.path.join(ROOT, "include", "mnt753_hip.h")).read()
    assert "#define MNT753_EINPUT (-7)" in text
    # the arithmetic-free ABI of the sanitizer builds has the same entry points
    stub = open(os.path.join(ROOT, "tools", "stub_abi", "stub_mnt753.cpp")).read()
    for s in CHECKS:
        assert f"int {s}(" in stub


def test_check_argument_errors(pkg):
    """null pointers and bad ids are MNT753_EINVAL, with or without a device"""
    L = pkg.lib()
    rep = pkg.CheckReport()
    buf = np.zeros(72, dtype=np.uint64)
    p = ctypes.c_void_p(buf.ctypes.data)
    EINVAL = -1
    assert L.mnt753_check_points(2, 1, p, 0, 1, ctypes.byref(rep), None) == EINVAL
    assert L.mnt753_check_points(0, 3, p, 0, 1, ctypes.byref(rep), None) == EINVAL
    assert L.mnt753_check_points(0, 1, None, 0, 1, ctypes.byref(rep), None) == EINVAL
    assert L.mnt753_check_points(0, 1, p, 0, 1, None, None) == EINVAL
    assert L.mnt753_check_scalars(-1, p, 0, 1, ctypes.byref(rep), None) == EINVAL
    assert L.mnt753_check_scalars(0, None, 0, 1, ctypes.byref(rep), None) == EINVAL
    assert L.mnt753_check_scalars(0, p, 0, 1, None, None) == EINVAL
    assert L.mnt753_check_products(5, p, p, p, 1, ctypes.byref(rep), None) == EINVAL
    assert L.mnt753_check_products(0, p, None, p, 1, ctypes.byref(rep), None) == EINVAL
    assert L.mnt753_check_products(0, p, p, p, 1, None, None) == EINVAL
    assert L.mnt753_r1cs_check(None, p, ctypes.byref(rep), None) == EINVAL
    assert b"check" in L.mnt753_last_error()


@pytest.mark.skipif(has_gpu(), reason="checks the no-device behaviour")
def test_checks_refuse_without_a_device(pkg):
    L = pkg.lib()
    rep = pkg.CheckReport()
    buf = np.zeros(72, dtype=np.uint64)
    p = ctypes.c_void_p(buf.ctypes.data)
    ENODEV = -2
    for n in (0, 1):
        assert L.mnt753_check_points(0, 1, p, 0, n, ctypes.byref(rep), None) == ENODEV
        assert L.mnt753_check_points(1, 2, p, 0, n, ctypes.byref(rep), None) == ENODEV
        assert L.mnt753_check_scalars(0, p, 0, n, ctypes.byref(rep), None) == ENODEV
        assert L.mnt753_check_products(1, p, p, p, n, ctypes.byref(rep), None) == ENODEV
    with pytest.raises(pkg.Mnt753Error):
        pkg.check_points(0, 1, buf[:24])
    with pytest.raises(pkg.Mnt753Error):
        pkg.check_scalars(0, buf[:12])


@pytest.mark.skipif(has_gpu(), reason="checks the no-device behaviour")
def test_check_cli_fails_loudly_without_gpu(tmp_path):
    params, inp, _ = G.e2e_paths(0)
    r = subprocess.run([EXE, "MNT4753", "check", params, inp], capture_output=True, text=True)
    assert r.returncode == 1 and "no HIP device" in r.stderr
    r = subprocess.run([EXE, "MNT4753", "check-r1cs", g16(0, "params.bin"), g16(0, "r1cs.bin"), g16(0, "witness.bin")], capture_output=True, text=True)
    assert r.returncode == 1 and "no HIP device" in r.stderr
    out = tmp_path / "o.bin"
    r = subprocess.run([EXE, "MNT4753", "compute", params, inp, str(out), "--validate"], capture_output=True, text=True)
    assert r.returncode == 1 and "no HIP device" in r.stderr and not out.exists()


def test_check_cli_usage():
    """a bare `check` is a usage error (2), like an unknown option or a missing file name"""
    params, inp, _ = G.e2e_paths(0)
    for args in (["MNT4753", "check"], ["MNT4753", "check-r1cs", params], ["MNT4753", "check", params, inp, inp], ["MNT4753", "check", params, "--frobnicate"],
                 ["BN128", "check", params]):
        r = subprocess.run([EXE] + args, capture_output=True, text=True)
        assert r.returncode == 2, (args, r.returncode, r.stderr)
    r = subprocess.run([EXE, "MNT4753", "compute", params, inp, "/dev/null", "--validated"], capture_output=True, text=True)
    assert r.returncode == 2 and "unknown option --validated" in r.stderr


# ---- the sanitizer binaries over the stub ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def asan():
    r = subprocess.run(["make", "asan"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return os.path.join(ROOT, "build", "san", "main_hip_asan")


def run_san(exe, args, expect_rc, extra_env=None, stdin=None):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", **(extra_env or {}))
    r = subprocess.run([exe] + args, capture_output=True, text=True, env=env, timeout=600, input=stdin)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == expect_rc, (args, r.returncode, r.stdout[-800:], r.stderr[-2000:])
    return r


@pytest.mark.parametrize("curve", [0, 1])
def test_check_modes_clean_under_asan(asan, curve, tmp_path):
    params, inp, _ = G.e2e_paths(curve)
    r = run_san(asan, [NAME[curve], "check", params], 0)
    for name in ("A", "B1", "B2", "L", "H"):
        assert f"{name}: " in r.stdout and "points ok" in r.stdout
    r = run_san(asan, [NAME[curve], "check", params, inp, "--gpus", "3"], 0)
    for name in ("w", "ca", "cb", "cc", "r"):
        assert f"{name}: " in r.stdout
    assert "rows satisfied" in r.stdout
    r = run_san(asan, [NAME[curve], "check-r1cs", g16(curve, "params.bin"), g16(curve, "r1cs.bin"), g16(curve, "witness.bin")], 0)
    assert "constraints: " in r.stdout
    # the stub told to report a bad point / an unsatisfied row: exit code 3, set, index and reason named
    r = run_san(asan, [NAME[curve], "check", params], 3, {"MNT753_STUB_BAD_POINT": "5"})
    assert "A: 1 bad, first at 5: off curve" in r.stdout and "H: 1 bad, first at 5: off curve" in r.stdout
    # (the stub answers per call, i.e. once per device slice: the counts add up, the lowest index in file order stays)
    r = run_san(asan, [NAME[curve], "check", params, "--gpus", "2"], 3, {"MNT753_STUB_BAD_POINT": "5"})
    assert "A: 2 bad, first at 5: off curve" in r.stdout
    r = run_san(asan, [NAME[curve], "check", params, inp], 3, {"MNT753_STUB_BAD_ROW": "2"})
    assert "constraint 2 of " in r.stdout and "is not satisfied" in r.stdout
    r = run_san(asan, [NAME[curve], "check-r1cs", g16(curve, "params.bin"), g16(curve, "r1cs.bin"), g16(curve, "witness.bin")], 3, {"MNT753_STUB_BAD_ROW": "1"})
    assert "constraint 1 of " in r.stdout


@pytest.mark.parametrize("curve", [0, 1])
def test_validate_option_clean_under_asan(asan, curve, tmp_path):
    params, inp, _ = G.e2e_paths(curve)
    out = tmp_path / "o"
    for flags in ([], ["--gpus", "3"], ["--repeat", "2"]):
        r = run_san(asan, [NAME[curve], "compute", params, inp, str(out), "--validate"] + flags, 0)
        assert "validate params" in r.stdout and "validate input" in r.stdout and out.exists()
        out.unlink()
    r = run_san(asan, [NAME[curve], "compute", params, inp, str(out)], 0, {"MNT753_VALIDATE": "1"})
    assert "validate params" in r.stdout
    out.unlink()
    r = run_san(asan, [NAME[curve], "compute", params, inp, str(out)], 0)
    assert "validate" not in r.stdout
    out.unlink()
    # a bad point in the parameters: nothing is proved, nothing written, exit code 3
    r = run_san(asan, [NAME[curve], "compute", params, inp, str(out), "--validate"], 3, {"MNT753_STUB_BAD_POINT": "0"})
    assert "A: 1 bad, first at 0: off curve" in r.stderr and not out.exists()
    # a bad row in a job's input: no output file for that job, exit code 3
    r = run_san(asan, [NAME[curve], "compute", params, inp, str(out), "--validate", "--gpus", "2"], 3, {"MNT753_STUB_BAD_ROW": "3"})
    assert "constraint 3 of " in r.stderr and not out.exists()
    # without the option the same environment proves as ever
    run_san(asan, [NAME[curve], "compute", params, inp, str(out)], 0, {"MNT753_STUB_BAD_ROW": "3", "MNT753_STUB_BAD_POINT": "0"})
    assert out.exists()
    # the resident prover goes on after a job that failed validation, and says so in the usual form
    feed = f"{inp} {tmp_path / 'a'}\n{inp} {tmp_path / 'b'}\n"
    r = run_san(asan, [NAME[curve], "compute", params, inp, str(out), "--serve", "--quiet", "--validate"], 3, {"MNT753_STUB_BAD_ROW": "0"}, stdin=feed)
    assert [l.split()[0] for l in r.stdout.strip().splitlines()] == ["failed", "failed", "failed"]
    assert not (tmp_path / "a").exists()
    d = lambda n: g16(curve, n)
    run_san(asan, [NAME[curve], "compute-r1cs", d("params.bin"), d("r1cs.bin"), d("witness.bin"), str(out), "--validate"], 0)
    run_san(asan, [NAME[curve], "complete", d("keys.bin"), d("input.bin"), d("challenge.bin"), str(tmp_path / "full"), "--validate"], 0)
    r = run_san(asan, [NAME[curve], "complete", d("keys.bin"), d("input.bin"), d("challenge.bin"), str(tmp_path / "full2"), "--validate"], 3, {"MNT753_STUB_BAD_POINT": "0"})
    assert "off curve" in r.stderr and not (tmp_path / "full2").exists()


# ---- the model against the reference's data ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve,params,inp", FIXTURES, ids=FIXTURE_IDS)
def test_model_calls_reference_parameter_files_well_formed(curve, params, inp):
    """every point of every set: every component below q and Curve.on_curve (or the all-zero-y identity); every scalar of the matching
    input below r; ca[i] cb[i] = cc[i] on every row (the generator's example system with its satisfying assignment)"""
    d, m, sets = V.params_sets(curve, params)
    for name, (group, _, n, pts) in sets.items():
        assert V.report(V.point_verdicts(curve, group, pts)) == (0, 0, V.OK), name
    vec = V.input_vectors(inp, d, m)
    for name, v in vec.items():
        assert V.report(V.scalar_verdicts(curve, v)) == (0, 0, V.OK), name
    assert V.report(V.product_verdicts(curve, vec["ca"], vec["cb"], vec["cc"])) == (0, 0, V.OK)


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("group", [1, 2])
def test_model_calls_libff_group_vectors_well_formed(curve, group):
    for rec in G.group(curve, group):
        for key in ("P", "Q", "sum", "dbl", "diff", "mul"):
            assert V.point_verdict(curve, group, rec[key]) == V.OK, key
        assert V.scalar_verdicts(curve, rec["s"]) == [V.OK]


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("group", [1, 2])
def test_model_rejects_what_it_should(curve, group):
    """the model is not vacuous: y + 1 is off the curve, x := q is not canonical, y = 0 is the identity whatever x holds"""
    cv, deg = V.CURVES[curve], V.degree(curve, group)
    P = G.group(curve, group)[0]["P"].copy()
    assert V.point_verdict(curve, group, P) == V.OK
    for k in range(2 * deg):
        bad = P.copy(); bad[12 * k] += np.uint64(1)
        assert V.point_verdict(curve, group, bad) == V.OFF_CURVE, k
    bad = P.copy(); bad[:12] = V.to_words([cv.q])[0]
    assert V.point_verdict(curve, group, bad) == V.NONCANONICAL
    bad[12 * deg] += np.uint64(1)
    assert V.point_verdict(curve, group, bad) == V.NONCANONICAL
    ident = P.copy(); ident[12 * deg:] = 0
    assert V.point_verdict(curve, group, ident) == V.OK
    assert V.scalar_verdicts(curve, V.to_words([0, 1, cv.r - 1, cv.r, cv.r + 1, (1 << 768) - 1])) == [0, 0, 0, 1, 1, 1]
