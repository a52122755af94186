"""GPU: subgroup membership of G2 on the device against the Python-integer reference of tests/subgroup_ref.py,
which tests/test_subgroup_cpu.py checks against the definition [r] P == O.  Every comparison is exact.

Shapes: one lane group per point or proof -- g = 32 per wave and 128 per workgroup on MNT4753, 21 and 84 on MNT6753 (lane 63 idles) --
so the sizes are 0, 1, 2, g, g + 1 and 4 g + 1 (one workgroup and one), and a point outside the subgroup sits at index 0, in the last
slot of a wave, in the first slot of the next one and at n - 1.  The points outside G2 are made here (designed_points.lift, their
cofactor parts [r] P, and Q + [r] P with Q in G2): once per process, shared by all tests."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import designed_points as DP
import subgroup_ref as S
import test_pairing_gpu as TP
from test_groth16_cpu import EXE, NAME

pytestmark = pytest.mark.gpu

G = S.GROUPS_PER_WAVE
SIZES = {c: [0, 1, 2, G[c], G[c] + 1, 4 * G[c] + 1] for c in (0, 1)}
W2 = {0: 48, 1: 72}


@functools.lru_cache(maxsize=None)
def pool(curve):
    """-> good [5, w2] (the generator and multiples), bad [9, w2] (lifted | cofactor parts | mixed), as wire words"""
    good = [S.CURVES[curve].gen(2)] + [S.generator_multiple(curve, k) for k in (2, 3, 0xABCDEF, S.CURVES[curve].r - 1)]
    off = S.off_subgroup_points(curve)
    bad = off["lifted"] + off["cofactor"] + off["mixed"]
    return np.stack([S.words(curve, p) for p in good]), np.stack([S.words(curve, p) for p in bad])


def good_batch(curve, n):
    return pool(curve)[0][np.arange(n) % 5].copy()


def edges(curve, n):
    return sorted({0, G[curve] - 1, G[curve], n - 1} & set(range(n)))


def raw(v):
    return np.array([(v >> (64 * i)) & (2 ** 64 - 1) for i in range(12)], dtype=np.uint64)


@pytest.mark.parametrize("curve", [0, 1])
def test_the_two_halves_vs_reference(gpu, curve):
    """psi(P) and [t - 1] P separately, so that a failure lies in the endomorphism or in the stepping"""
    C = S.CURVES[curve]
    off = S.off_subgroup_points(curve)
    pts = [C.gen(2), C.neg(C.gen(2)), S.generator_multiple(curve, 7), S.generator_multiple(curve, C.r - 2)]
    pts += off["lifted"] + off["cofactor"][:1] + off["mixed"][:1] + [pt for _, pt in DP.sparse_points(curve)]
    w = np.stack([S.words(curve, p) for p in pts])
    got = gpu.api.test_g2_endomorphism(curve, w)
    assert np.array_equal(got, np.stack([S.words(curve, S.psi(curve, p)) for p in pts]))
    got = gpu.api.test_g2_loop_multiple(curve, w)
    want = np.stack([S.words(curve, S.loop_multiple(curve, p)) for p in pts])
    assert np.array_equal(got, want)
    # the members are exactly those where the halves agree
    same = [np.array_equal(a, b) for a, b in zip(want, np.stack([S.words(curve, S.psi(curve, p)) for p in pts]))]
    assert same == [S.in_subgroup(curve, p) for p in pts] and same[:4] == [True] * 4 and not any(same[4:])


@pytest.mark.parametrize("curve,n", [(c, n) for c in (0, 1) for n in SIZES[c]])
def test_check_subgroup_sizes_and_positions(gpu, curve, n):
    bad = pool(curve)[1]
    pts = good_batch(curve, n)
    assert gpu.check_subgroup(curve, 2, pts.reshape(-1) if n else np.zeros(0, dtype=np.uint64), n=n) == (0, 0, 0)
    if n == 0:
        return
    for k, i in enumerate(edges(curve, n)):
        one = pts.copy()
        one[i] = bad[k % len(bad)]
        assert gpu.check_subgroup(curve, 2, one) == (1, i, gpu.BAD_NOT_IN_SUBGROUP), (n, i)
        assert gpu.check_points(curve, 2, one) == (0, 0, 0)                # is_well_formed() alone still calls them good
    allbad = bad[np.arange(n) % len(bad)].copy()
    dev = gpu.DeviceBuffer.from_numpy(allbad)
    assert gpu.check_subgroup(curve, 2, dev.ptr.value, on_device=True, n=n) == (n, 0, gpu.BAD_NOT_IN_SUBGROUP)
    several = pts.copy()
    for i in edges(curve, n):
        several[i] = bad[(3 + i) % len(bad)]
    dev = gpu.DeviceBuffer.from_numpy(several)
    assert gpu.check_subgroup(curve, 2, dev.ptr.value, on_device=True, n=n) == (len(edges(curve, n)), 0, gpu.BAD_NOT_IN_SUBGROUP)


@pytest.mark.parametrize("curve", [0, 1])
def test_check_subgroup_precedence_per_point(gpu, curve):
    """a non-canonical point, an off-curve point, an identity and an off-subgroup point in one batch, each of the three bad ones
    first once: first_bad / first_reason are the lowest index's, and the identity is good"""
    C = S.CURVES[curve]
    w2, (good, bad) = W2[curve], pool(curve)
    noncanon = good[1].copy(); noncanon[w2 - 12:w2] = raw(C.q)             # the last component of y = q: another lane's flag
    offcurve = good[2].copy(); offcurve[12] ^= np.uint64(1)
    ident = good[3].copy(); ident[w2 // 2:] = 0
    # a point that is BOTH non-canonical and outside the subgroup is non-canonical; off the twist and (as any such point) outside: off curve
    both = bad[0].copy(); both[:12] = raw(C.q + 5)
    kinds = {"nc": (noncanon, gpu.BAD_NONCANONICAL), "oc": (offcurve, gpu.BAD_OFF_CURVE), "sg": (bad[4], gpu.BAD_NOT_IN_SUBGROUP)}
    n = G[curve] + 3
    for order in (("nc", "oc", "sg"), ("oc", "sg", "nc"), ("sg", "nc", "oc")):
        pts = good_batch(curve, n)
        pts[1] = ident
        slots = (2, G[curve] - 1, G[curve] + 1)
        for slot, kind in zip(slots, order):
            pts[slot] = kinds[kind][0]
        assert gpu.check_subgroup(curve, 2, pts) == (3, 2, kinds[order[0]][1]), order
    assert gpu.check_subgroup(curve, 2, np.stack([ident, both])) == (1, 1, gpu.BAD_NONCANONICAL)
    assert gpu.check_subgroup(curve, 2, np.stack([ident, ident])) == (0, 0, 0)


@pytest.mark.parametrize("curve", [0, 1])
def test_check_subgroup_on_g1_is_check_points(gpu, curve):
    pts = gpu.synth_points(curve, 1, 5, 40)
    assert gpu.check_subgroup(curve, 1, pts) == gpu.check_points(curve, 1, pts) == (0, 0, 0)
    pts[17, 12] ^= np.uint64(1)
    pts[30, :12] = raw(S.CURVES[curve].q)
    assert gpu.check_subgroup(curve, 1, pts) == gpu.check_points(curve, 1, pts) == (2, 17, gpu.BAD_OFF_CURVE)
    assert gpu.check_subgroup(curve, 1, np.zeros(0, dtype=np.uint64), n=0) == (0, 0, 0)


# ---- verification ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bad_b(curve):
    """replacements for B of the fixture's proof: B + [r] P for two lifted P, and a lifted point itself"""
    C = S.CURVES[curve]
    proof = TP.g16_key_parts(curve)[4]
    B = S.from_words(curve, proof[24:24 + W2[curve]])
    off = S.off_subgroup_points(curve)
    return np.stack([S.words(curve, C.add(B, off["cofactor"][0], 2)), S.words(curve, off["lifted"][1]), S.words(curve, C.add(B, off["cofactor"][2], 2))])


def build_batch(curve, n):
    """-> proofs, inputs, verdicts with the flag, verdicts without it"""
    w2 = W2[curve]
    good, _ = TP.proof_pool(curve)
    inp = TP.g16_key_parts(curve)[5]
    proofs, inputs = good[np.arange(n) % TP.NP].copy(), np.tile(inp, (n, 1))
    on, off = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    taken = set(edges(curve, n))
    for k, i in enumerate(edges(curve, n)):
        proofs[i, 24:24 + w2] = bad_b(curve)[k % 3]
        on[i], off[i] = 3, 2
        if i + 1 < n and i + 1 not in taken:                                 # a malformed neighbour: the identity as A, or B off the twist
            taken.add(i + 1)
            if k % 2 == 0:
                proofs[i + 1, :24] = 0
            else:
                proofs[i + 1, 24 + 12] ^= np.uint64(1)
            on[i + 1] = off[i + 1] = 1
        if i + 2 < n and i + 2 not in taken:                                 # a wrong C: the pairing check fails, B is fine
            taken.add(i + 2)
            proofs[i + 2, 24 + w2:] = proofs[i + 2, :24]
            on[i + 2] = off[i + 2] = 2
    return proofs, inputs, on, off


def plain_verify(gpu, vk, proofs, inputs):
    """mnt753_groth16_verify itself, the entry that never returns 3"""
    p, x = np.ascontiguousarray(proofs, dtype=np.uint64), np.ascontiguousarray(inputs, dtype=np.uint64)
    v = np.zeros(len(p), dtype=np.uint8)
    rc = gpu.lib().mnt753_groth16_verify(vk._h, ctypes.c_void_p(p.ctypes.data), ctypes.c_void_p(x.ctypes.data), len(p), 0, ctypes.c_void_p(v.ctypes.data), None)
    assert rc == int(np.count_nonzero(v))
    return v


@pytest.mark.parametrize("curve,n", [(c, n) for c in (0, 1) for n in SIZES[c][1:]])
def test_verify_with_and_without_the_flag(gpu, curve, n):
    alpha, beta, delta, abc, _, _ = TP.g16_key_parts(curve)
    vk = gpu.VerificationKey(curve, alpha, beta, delta, abc)
    assert vk.check_subgroup() == (0, 0, 0)
    good, _ = TP.proof_pool(curve)
    inp = TP.g16_key_parts(curve)[5]
    valid, vin = good[np.arange(n) % TP.NP], np.tile(inp, (n, 1))
    assert list(vk.verify(valid, vin, check_subgroup=True)) == [0] * n
    proofs, inputs, on, off = build_batch(curve, n)
    assert list(vk.verify(proofs, inputs, check_subgroup=True)) == list(on)
    assert list(vk.verify(proofs, inputs)) == list(off)
    assert list(plain_verify(gpu, vk, proofs, inputs)) == list(off)
    if n == G[curve] + 1:                                                    # from device memory, and an unknown flag bit
        dp, di = gpu.DeviceBuffer.from_numpy(proofs), gpu.DeviceBuffer.from_numpy(inputs)
        assert list(vk.verify(dp.ptr.value, di.ptr.value, on_device=True, n=n, check_subgroup=True)) == list(on)
        v = np.zeros(n, dtype=np.uint8)
        assert gpu.lib().mnt753_groth16_verify_ex(vk._h, dp.ptr, di.ptr, n, 1, 6, ctypes.c_void_p(v.ctypes.data), None) == -1
    vk.close()
    if n == 2:                                                               # a key whose delta_g2 is outside G2 is still a key; its check says so
        other = gpu.VerificationKey(curve, alpha, beta, bad_b(curve)[0], abc)
        assert other.check_subgroup() == (1, 1, gpu.BAD_NOT_IN_SUBGROUP)
        other.close()


# ---- the command line -------------------------------------------------------------------------------------------------------------------
def cli(args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True)


@pytest.mark.parametrize("curve", [0, 1])
def test_cli_check_subgroup(gpu, curve, tmp_path):
    src = TP.g16(curve, "params.bin")
    raw_bytes = bytearray(open(src, "rb").read())
    d, m = np.frombuffer(raw_bytes[:16], dtype="<u8")
    assert m + 1 > 3
    at = 16 + 2 * 8 * 24 * (int(m) + 1) + 3 * 8 * W2[curve]                  # B2[3]
    raw_bytes[at:at + 8 * W2[curve]] = pool(curve)[1][1].astype("<u8").tobytes()
    path = tmp_path / "params.bin"
    path.write_bytes(bytes(raw_bytes))
    r = cli([NAME[curve], "check", path, "--subgroup"])
    assert r.returncode == 3 and "B2: 1 bad, first at 3: not in the subgroup" in r.stdout.splitlines(), r.stdout + r.stderr
    r = cli([NAME[curve], "check", path])
    assert r.returncode == 0 and "bad" not in r.stdout, r.stdout + r.stderr
    r = cli([NAME[curve], "check", src, "--subgroup", "--gpus", "1"])
    assert r.returncode == 0 and "bad" not in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("curve", [0, 1])
def test_cli_verify_check_subgroup(gpu, curve, tmp_path):
    w2 = W2[curve]
    el = TP.g16_elements_file(curve, tmp_path)
    inp, full = TP.g16(curve, "input.bin"), TP.g16(curve, "full.bin")
    proof = np.fromfile(full, dtype="<u8")
    proof[24:24 + w2] = bad_b(curve)[0]
    forged = tmp_path / "forged.bin"
    proof.astype("<u8").tofile(forged)
    r = cli([NAME[curve], "verify", el, inp, full, forged, "--check-subgroup"])
    assert r.returncode == 3 and r.stdout.splitlines() == ["VERIFIED", "REJECTED (B not in the subgroup)"], r.stdout + r.stderr
    r = cli([NAME[curve], "verify", el, inp, full, forged])
    assert r.returncode == 3 and r.stdout.splitlines() == ["VERIFIED", "REJECTED"]
    r = cli([NAME[curve], "verify", el, inp, full, "--check-subgroup"])
    assert r.returncode == 0 and r.stdout.splitlines() == ["VERIFIED"]
    words = np.fromfile(el, dtype="<u8")
    words[24 + w2:24 + 2 * w2] = pool(curve)[1][0]                           # delta_g2 := a lifted point
    badkey = tmp_path / "bad_elements.bin"
    words.astype("<u8").tofile(badkey)
    r = cli([NAME[curve], "verify", badkey, inp, full, "--check-subgroup"])
    assert r.returncode == 3 and r.stdout == "" and "delta_g2 of the key: not in the subgroup" in r.stderr, r.stdout + r.stderr
