"""CPU: the host model of the group inversion (fp_inv_integer_group, csrc/fp_inv.hip.h) -- one Bernstein-Yang inversion computed
limb-parallel by 8, 16 or 32 lanes.  tools/host_inv_group_check.cpp runs the routine's own __host__ __device__ per-lane arithmetic with
the lanes as an array index and the exchange as array reads: bit-identical to fp_inv_integer and confirmed by the host field's
independent inversion on 0, 1, 2, p - 1, p - 2, (p +- 1) / 2, R' mod p, 2^k for every k < 753, inputs whose low 28, 56 and 84 bits are
zero and 10^5 seeded random inputs per modulus (G = 16; a fifth of that for G = 8 and 32), with the limb ranges stated above the routine
asserted after every one of the 78 batches.  Built without a sanitizer here (about a minute of one core)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_group_inversion_host_model(tmp_path):
    exe = tmp_path / "host_inv_group_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tools", "host_inv_group_check.cpp")], check=True, timeout=600)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=1200, cwd=ROOT)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout + out.stderr
