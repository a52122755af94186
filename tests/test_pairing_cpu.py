"""CPU: the pairing's constants, the Python-integer model of tests/pairing_ref.py against the reference's GT elements and proofs,
the layout of a serialised verification key, the new symbols of the C ABI, and the project's own tower and pairing code compiled for
the host (tools/host_pairing_check.cpp)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import keygen_ref as K
import oracle_lib as O
import pairing_ref as PR
import pyref
from test_abi_cpu import header_symbols

ROOT = O.ROOT
NEW_SYMBOLS = ["mnt753_gt_words", "mnt753_pairing", "mnt753_vk_create", "mnt753_vk_destroy", "mnt753_vk_num_inputs", "mnt753_vk_coefficient_bytes", "mnt753_vk_set_workspace_cap", "mnt753_vk_gt",
               "mnt753_vk_serialize", "mnt753_vk_accumulate", "mnt753_groth16_verify"]
NEW_TEST_SYMBOLS = ["mnt753_test_tower_op", "mnt753_test_miller_loop"]


@pytest.mark.parametrize("curve", [0, 1])
def test_derived_constants(curve):
    c = PR.constants(curve)
    q, r, k = c["q"], c["r"], c["k"]
    assert c["phi"] == (q * q + 1 if k == 4 else q * q - q + 1) and c["phi"] % r == 0
    assert (q ** k - 1) % r == 0 and all((q ** j - 1) % r for j in range(1, k))          # k is the embedding degree
    assert c["loop_count"].bit_length() == 377 and bin(c["loop_count"]).count("1") == 175
    assert c["loop_neg"] == (curve == 0)
    w0 = -c["w0_abs"] if c["w0_neg"] else c["w0_abs"]
    assert w0 == (-(c["loop_count"] - 1) if curve == 0 else c["loop_count"])
    assert (q + w0) * r == c["phi"]                                                       # the last chunk is w1 q + w0 with w1 = 1
    assert all(pow(g, k, q) == 1 for g in c["gamma"]) and c["gamma"][0] == 1
    assert pow(c["gamma"][1], k // 2, q) == q - 1                                         # a primitive k-th root: NR is no square


def test_generated_header_is_current(tmp_path):
    """csrc/mnt753_pairing_constants.h is what tools/gen_constants.py derives, and it holds the model's constants"""
    import gen_constants as GC
    for curve in (0, 1):
        a, b = GC.pairing_constants(curve), PR.constants(curve)
        assert (a["loop"], a["loop_neg"], a["w0_abs"], a["w0_neg"], a["frob"]) == (b["loop_count"], b["loop_neg"], b["w0_abs"], b["w0_neg"], b["frob"])
    text = open(os.path.join(ROOT, "snark-challenge-prover-reference_amd", "csrc", "mnt753_pairing_constants.h")).read()
    words = GC.arr(GC.limbs(PR.constants(1)["loop_count"], 12, 32))
    assert text.count(words) == 3                          # the loop count of both curves (the same number) and |w0| of MNT6753


@pytest.mark.parametrize("name", PR.VK_DIRS)
def test_model_pairing_is_the_references(name):
    P = PR.Pairing(PR.dir_curve(name))
    a, b = PR.alpha_beta_words(name)
    assert np.array_equal(P.pair_words(a, b), PR.vk_head(name))


@pytest.mark.parametrize("curve", [0, 1])
def test_model_accepts_the_fixture_proof_and_rejects_c_replaced_by_a(curve):
    name = f"g16_mnt{4 if curve == 0 else 6}"
    P = PR.Pairing(curve)
    C = P.C
    w2 = 24 * C.deg
    raw = open(os.path.join(PR.GOLDEN, name, "vk.txt"), "rb").read()
    pos = 8 * w2 + 1 + 8 * w2
    ints = lambda b: [int(v) for v in np.frombuffer(b, dtype="<u8")]
    abc = [C.affine_from_words(ints(raw[pos + 1:pos + 193]), 1), C.affine_from_words(ints(raw[pos + 202:pos + 394]), 1)]
    delta = C.affine_from_words([int(v) for v in PR.delta_words(name)], 2)
    proof = [int(v) for v in np.fromfile(os.path.join(PR.GOLDEN, name, "full.bin"), dtype="<u8")]
    A, B, Cp = C.affine_from_words(proof[:24], 1), C.affine_from_words(proof[24:24 + w2], 2), C.affine_from_words(proof[24 + w2:], 1)
    inp = np.fromfile(os.path.join(PR.GOLDEN, name, "input.bin"), dtype="<u8", count=24)
    assert C.fr_from_words([int(v) for v in inp[:12]]) == 1
    x = [C.fr_from_words([int(v) for v in inp[12:]])]
    ab = P.gt_from_words(PR.vk_head(name))
    assert P.groth16_verify(ab, delta, abc, (A, B, Cp), x)
    assert not P.groth16_verify(ab, delta, abc, (A, B, A), x)


@pytest.mark.parametrize("fixture", K.FIXTURES, ids=K.fixture_id)
def test_serialised_key_layout(fixture):
    """GT | '0' delta_g2 | '0' ABC[0] | the sparse vector of the rest: vk_elements.bin and the model's GT give the reference's vk.txt"""
    curve, tag = fixture
    d = K.fixture_dir(curve, tag)
    el = np.fromfile(os.path.join(d, "vk_elements.bin"), dtype="<u8").astype(np.uint64)
    w2 = K.aff_words(curve, 2)
    gt = PR.Pairing(curve).pair_words(el[:24], el[24:24 + w2])
    want = open(os.path.join(d, "vk.txt"), "rb").read()
    assert PR.serialize_vk(curve, gt, el[24 + w2:24 + 2 * w2], el[24 + 2 * w2:]) == want
    assert len(want) == (1163, 1547)[curve]


def test_new_symbols_are_declared_and_exported(pkg):
    L = ctypes.CDLL(pkg.lib_path())
    declared = header_symbols()
    for s in NEW_SYMBOLS:
        assert s in declared and hasattr(L, s), s
    T = pkg.test_lib()
    declared = header_symbols("mnt753_hip_test.h")
    for s in NEW_TEST_SYMBOLS:
        assert s in declared and hasattr(T, s), s
    assert [pkg.gt_words(c) for c in (0, 1, 2)] == [48, 72, 0]
    assert pkg.lib().mnt753_vk_gt(None, None) == -1 and pkg.lib().mnt753_vk_destroy(None) == 0


def has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.mark.skipif(has_gpu(), reason="checks the no-device behaviour")
def test_no_device_no_pairing(pkg):
    g1 = np.zeros(24, dtype=np.uint64)
    g2 = np.zeros(48, dtype=np.uint64)
    with pytest.raises(pkg.Mnt753Error, match="no HIP device"):
        pkg.pairing(0, g1, g2)
    with pytest.raises(pkg.Mnt753Error, match="no HIP device"):
        pkg.VerificationKey(0, g1, g2, g2, np.zeros(48, dtype=np.uint64))


def test_tower_and_pairing_compiled_for_the_host(tmp_path):
    """tools/host_pairing_check.cpp: the tower identities on random elements and the whole reduced pairing of the six committed keys
    through the one-lane fields -- the same source the device instantiates with its lane-split fields"""
    exe = tmp_path / "host_pairing_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tools", "host_pairing_check.cpp")], check=True, timeout=600)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout + out.stderr


EXE = os.path.join(ROOT, "snark-challenge-prover-reference_amd", "main_hip")


def cli(args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True)


def test_cli_usage_errors_exit_2(tmp_path):
    el = os.path.join(K.fixture_dir(0, "cut21"), "vk_elements.bin")
    for args in (["MNT4753", "vk"], ["MNT4753", "vk", el], ["MNT4753", "vk", el, tmp_path / "o", "extra"], ["MNT4753", "verify", el],
                 ["MNT4753", "verify", el, "input"], ["MNT4753", "verify", el, "input", "proof", "--what"], ["MNT5", "vk", el, tmp_path / "o"]):
        r = cli(args)
        assert r.returncode == 2, (args, r.stderr)
    assert "usage" in cli(["MNT6753", "verify"]).stderr
    assert "pairing" in cli(["MNT4753", "generate"]).stderr and "vk <vk_elements.bin>" in cli(["MNT4753", "generate"]).stderr
    assert not (tmp_path / "o").exists()


@pytest.mark.skipif(has_gpu(), reason="checks the no-device behaviour")
@pytest.mark.parametrize("curve", [0, 1])
def test_cli_fails_loudly_without_gpu(curve, tmp_path):
    name = ("MNT4753", "MNT6753")[curve]
    d = K.fixture_dir(curve, "cut21")
    g = os.path.join(PR.GOLDEN, f"g16_mnt{4 if curve == 0 else 6}")
    r = cli([name, "vk", os.path.join(d, "vk_elements.bin"), tmp_path / "vk.txt"])
    assert r.returncode == 1 and "no HIP device" in r.stderr
    assert not (tmp_path / "vk.txt").exists()
    r = cli([name, "verify", os.path.join(d, "vk_elements.bin"), os.path.join(g, "input.bin"), os.path.join(g, "full.bin")])
    assert r.returncode == 1 and "no HIP device" in r.stderr and r.stdout == ""


def test_tower_and_pairing_on_the_host_under_sanitizers():
    """`make asan` also builds tools/host_pairing_check.cpp with -fsanitize=address,undefined: a stand-alone program, run directly"""
    r = subprocess.run(["make", "build/san/host_pairing_check_asan"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    out = subprocess.run([os.path.join(ROOT, "build", "san", "host_pairing_check_asan")], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0 and "ALL OK" in out.stdout and "runtime error" not in out.stderr, out.stdout + out.stderr
