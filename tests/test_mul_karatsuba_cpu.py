"""CPU: the signed product with a Karatsuba product half (fp_mul_s_k / fp_mul_s_ip_k, csrc/fp753.hip.h) on the host, under
AddressSanitizer + UBSan.  tools/host_karatsuba_check.cpp compiles the routines' own __host__ __device__ source and compares them with
fp_mul_s limb for limb on both moduli: 3000 seeded random pairs inside the operand contract per modulus, every limb at 0, 2^28 - 1 and
+-(2^29 - 1), the halves at opposite extremes in both operands (the patterns that maximise the middle term), the top limb at its
negative end, the values 0, p and 2p - 1, both argument orders, both entry points; every column is recomputed in __int128 and must
satisfy |column| < 2^63, inside the contract every partial sum of a column too.  Then the Python model the GPU test compares with
(tests/mul_karatsuba_ref.py) against the host twin of the raw ops on the same edge vectors, and the two op codes against the header."""
import os
import random
import subprocess

import numpy as np

import field_raw_ref as F
import mul_karatsuba_ref as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_karatsuba_product_host_model(tmp_path):
    exe = tmp_path / "host_karatsuba_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-o", str(exe), os.path.join(ROOT, "tools", "host_karatsuba_check.cpp")], check=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-3000:]
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout + out.stderr


def test_op_codes_are_the_header_s():
    """appended behind FR_INV_GROUP; every earlier op keeps its number"""
    codes = K.header_codes()
    assert codes["FR_MUL_S_K"] == K.OP_MUL_S_K and codes["FR_MUL_S_IP_K"] == K.OP_MUL_S_IP_K and codes["FR_INV_GROUP"] == 24
    assert [codes["FR_" + n.upper()] for n in F.OP_NAMES] == list(range(len(F.OP_NAMES)))
    assert codes["FR_NUM_OPS"] == K.OP_MUL_S_IP_K + 1


def test_python_model_against_the_host_twin(tmp_path):
    """the raw ops compiled with g++ (the same source as the device hook): the two new ops give fp_mul_s's limbs and the limbs the
    Python integers predict, on the edge vectors and 256 random records per modulus"""
    twin = F.build_host_twin(tmp_path)
    for mod in (0, 1):
        p = F.MODS[mod]
        pairs = K.edge_pairs(p) + K.random_pairs(p, random.Random(8 + mod), 256)
        rec = K.records(pairs)
        want = K.expected_limbs(pairs, p)
        plain = twin(mod, F.MUL_S, rec, 0)
        assert np.array_equal(plain[:, :F.NL], want), f"modulus {mod}: the Python model is not fp_mul_s"
        for op in (K.OP_MUL_S_K, K.OP_MUL_S_IP_K):
            got = twin(mod, op, rec, 0)
            bad = np.flatnonzero((got[:, :F.NL] != want).any(axis=1))
            assert bad.size == 0, f"modulus {mod}, op {op}: {bad.size} of {len(pairs)} records differ, first at {bad[:8]}"
        assert np.array_equal(got[:, F.NL:2 * F.NL], rec[:, :F.NL]), f"modulus {mod}: fp_mul_s_ip_k changed the operand it keeps"
