"""The folded verification with one tail per segment without a GPU: the host-side plan of segments, chunks and
rechecked runs (csrc/fold_locate_plan.hpp) compiled stand-alone, plainly and under AddressSanitizer + UBSan, and the per-segment
equation in the Python-integer model of tests/fold_ref.py with a model segment size of 2.  tests/test_fold_locate_gpu.py pins the
device."""
import functools
import os
import subprocess

import pytest

import fold_ref as FR
import oracle_lib as O
from test_abi_cpu import exported, header_symbols

ROOT = O.ROOT
RHO = [0x9F3A7C2E51B84D06A1C3E5F708192A3B, 0x4D1E6F8092A3B4C5D6E7F8091A2B3C4D, 0x7B5C3D1E0F2A4B6C8D9EAFB0C1D2E3F5]   # fixed 128-bit coefficients
SEG = 2                                                                      # the model's segment size


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]],
                         ids=["plain", "asan_ubsan"])
def test_the_plan_on_its_own(tmp_path, flags):
    """segment ranges at n = 1, g - 1, g, g + 1, 2 g + 1 for both g; chunks under caps below one segment, of exactly one, of one and
    a half and beyond n; runs for none, all, alternating, first only and last only rejected"""
    exe = tmp_path / "host_fold_locate_plan_check"
    subprocess.run(["g++", "-std=c++17"] + flags + ["-o", str(exe), os.path.join(ROOT, "tools", "host_fold_locate_plan_check.cpp")], check=True, timeout=600)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout + out.stderr


def test_new_entry_points_are_declared_exported_and_bound(pkg):
    declared = set(header_symbols())
    prod = exported(pkg.lib_path())
    L = pkg.lib()
    for name in ("mnt753_fold_segment_proofs", "mnt753_groth16_verify_folded_locate"):
        assert name in declared, f"{name} is not declared in include/mnt753_hip.h"
        assert name in prod, f"{name} is not exported by the product library"
        assert getattr(L, name).argtypes is not None, f"{name} is missing from the Python signature table"
    assert "mnt753_test_fold_segment_parts" in header_symbols("mnt753_hip_test.h")
    assert "mnt753_test_fold_segment_parts" in exported(pkg.api.test_lib_path())
    assert (pkg.fold_segment_proofs(0), pkg.fold_segment_proofs(1), pkg.fold_segment_proofs(7)) == (128, 84, 0)


@functools.lru_cache(maxsize=None)
def batch(curve):
    """the fixture proof and two re-randomised copies of it, their inputs"""
    C = FR.model(curve).C
    _, _, _, _, proof, inp = FR.g16_words(curve)
    p0 = FR.proof_from_words(curve, proof)
    x = [C.fr_from_words([int(v) for v in inp])]
    return [p0, FR.rerandomised(curve, p0, 0x1234567), FR.rerandomised(curve, p0, 0x7654321)], [x, x, x]


def segments(proofs, inputs, rhos):
    """the model's segments: (proofs, inputs, coefficients) of every run of SEG proofs"""
    return [(proofs[a:a + SEG], inputs[a:a + SEG], rhos[a:a + SEG]) for a in range(0, len(proofs), SEG)]


@pytest.mark.parametrize("curve", [0, 1])
def test_the_segments_parts_make_up_the_batch(curve):
    """prod F_s = F, sum T_s = T, sum rho_s = rho, with FR.parts on the subsets; and every segment of a valid batch is accepted"""
    P = FR.model(curve)
    C = P.C
    key = FR.g16_key(curve)
    proofs, inputs = batch(curve)
    whole = FR.parts(key, proofs, inputs, RHO)
    per = [FR.parts(key, *s) for s in segments(proofs, inputs, RHO)]
    assert len(per) == 2
    assert FR.product(curve, [p["F"] for p in per]) == whole["F"]
    assert C.add(per[0]["T"], per[1]["T"], 1) == whole["T"]
    assert (per[0]["rho"] + per[1]["rho"]) % C.r == whole["rho"]
    assert per[0]["rho"] == RHO[0] + RHO[1] < 2 ** 129 and per[1]["rho"] == RHO[2]
    assert C.add(per[0]["S"], per[1]["S"], 1) == whole["S"]
    assert all(FR.verdict(key, p) for p in per)


@pytest.mark.parametrize("curve", [0, 1])
def test_a_cancelling_pair_is_found_only_across_a_boundary(curve):
    """C_0 + D and C_1 - D with rho = (1, 1): one segment that holds both accepts them (the documented limit of predictable
    coefficients); with the boundary between them both segments are rejected"""
    C = FR.model(curve).C
    key = FR.g16_key(curve)
    proofs, inputs = batch(curve)
    D = C.mul(0xD15EA5E, C.gen(1), 1)
    b0 = (proofs[0][0], proofs[0][1], C.add(proofs[0][2], D, 1))
    b1 = (proofs[1][0], proofs[1][1], C.add(proofs[1][2], C.neg(D), 1))
    inside = [FR.accepts(key, *s) for s in segments([b0, b1, proofs[2]], inputs, [1, 1, RHO[2]])]
    assert inside == [True, True]
    across = [FR.accepts(key, *s) for s in segments([proofs[2], b0, b1], inputs, [RHO[2], 1, 1])]
    assert across == [False, False]
