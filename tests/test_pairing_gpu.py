"""GPU: the tower, the Miller loop, the final exponentiation, mnt753_pairing and Groth16 verification on the device against the
Python-integer model of tests/pairing_ref.py and the reference's own GT elements (the heads of tests/golden/*/vk.txt).  Every
comparison is of all words; there is no tolerance.

Shapes: one lane group per pairing -- 32 groups per wave and 128 per workgroup on MNT4753, 21 and 84 on MNT6753 (lane 63 idles) -- so
the batches are 1, 2, a full wave, a wave and one, and a workgroup and one (two workgroups on MNT6753).  Batches cycle 7 distinct
pairs, which keeps the model at 7 pairings per curve."""
import functools
import os

import numpy as np
import pytest

import keygen_ref as K
import oracle_lib as O
import pairing_ref as PR
import pyref

pytestmark = pytest.mark.gpu

SIZES = {0: [1, 2, 32, 33, 129], 1: [1, 21, 22, 85, 86]}
WAVE = {0: 32, 1: 21}
NP = 7


@functools.lru_cache(maxsize=None)
def model(curve):
    return PR.Pairing(curve)


def rand_elems(curve, seed, n):
    """n random tower elements (integers) and the specials 0, 1, u, v and every single-component element"""
    P = model(curve)
    rng = pyref.splitmix64(seed)
    d, q = P.deg, P.q
    out = [tuple(tuple(pyref.rand_below(rng, q) for _ in range(d)) for _ in range(2)) for _ in range(n)]
    z = (0,) * d
    unit = lambda h, c, v=1: tuple(tuple(v if (hh == h and cc == c) else 0 for cc in range(d)) for hh in range(2))
    out += [(z, z), unit(0, 0), unit(0, 1), unit(1, 0)]
    out += [unit(h, c, pyref.rand_below(rng, q)) for h in range(2) for c in range(d)]
    return out


def words(curve, elems):
    P = model(curve)
    return np.stack([P.gt_to_words(e) for e in elems])


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("curve", [0, 1])
def test_tower_operations_vs_model(gpu, curve, split):
    """mul, sqr, inv, the unitary inverse and every Frobenius map on 64 random elements and the specials: more than a wave of
    one-lane elements, more than two waves of lane groups (the idle lane 63 of MNT6753 included)."""
    P = model(curve)
    a = rand_elems(curve, 100 + curve, 64)
    b = list(reversed(a))
    wa, wb = words(curve, a), words(curve, b)
    zero = (P.f_zero, P.f_zero)
    cases = [(0, [P.mul(x, y) for x, y in zip(a, b)]), (1, [P.sqr(x) for x in a]),
             (2, [zero if x == zero or P.C.f_is_zero(P.C.f_sub(P.f_sqr(x[0]), P.f_mul_by_u(P.f_sqr(x[1])))) else P.inv(x) for x in a]),
             (3, [P.conj(x) for x in a])]
    cases += [(10 + i, [P.frobenius(x, i) for x in a]) for i in range(1, P.k)]
    for op, want in cases:
        got = gpu.api.test_tower_op(curve, split, op, wa, wb)
        assert np.array_equal(got, words(curve, want)), (curve, split, op)


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("curve", [0, 1])
def test_w0_power_and_final_exponentiation_vs_model(gpu, curve, split):
    """the |w0| power of the last chunk on the 64 random elements and the specials of the other tower operations -- a full wave of lane
    groups, the group beside the idle lane 63 of MNT6753, a second and a third wave -- and the whole final exponentiation on random
    elements"""
    P = model(curve)
    a = rand_elems(curve, 100 + curve, 64)
    got = gpu.api.test_tower_op(curve, split, 4, words(curve, a))
    assert np.array_equal(got, words(curve, [P.pow(x, P.K["w0_abs"]) for x in a]))
    a = a[:6]
    got = gpu.api.test_tower_op(curve, split, 5, words(curve, a))
    assert np.array_equal(got, words(curve, [P.final_exponentiation(x) for x in a]))


@functools.lru_cache(maxsize=None)
def pairs(curve):
    """NP distinct (P, Q) pairs, their unreduced Miller values and their pairings from the model"""
    from __graft_entry__ import load_package
    pkg = load_package()
    P = model(curve)
    g1 = pkg.synth_points(curve, 1, 71, NP)
    g2 = pkg.synth_points(curve, 2, 72, NP)
    ml, gt = [], []
    for p, q in zip(g1, g2):
        f = P.miller(P.C.affine_from_words([int(v) for v in p], 1), P.C.affine_from_words([int(v) for v in q], 2))
        ml.append(P.gt_to_words(f))
        gt.append(P.gt_to_words(P.final_exponentiation(f)))
    return g1, g2, np.stack(ml), np.stack(gt)


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("curve", [0, 1])
def test_unreduced_miller_value_vs_model(gpu, curve, split):
    g1, g2, ml, _ = pairs(curve)
    assert np.array_equal(gpu.api.test_miller_loop(curve, split, g1, g2), ml)


@pytest.mark.parametrize("name", PR.VK_DIRS)
def test_pairing_of_the_golden_keys(gpu, name):
    """e(alpha_g1, beta_g2) of the six committed keys is the GT element the reference wrote at the head of vk.txt"""
    curve = PR.dir_curve(name)
    a, b = PR.alpha_beta_words(name)
    assert gpu.gt_words(curve) == (48, 72)[curve]
    assert np.array_equal(gpu.pairing(curve, a, b)[0], PR.vk_head(name))


@pytest.mark.parametrize("curve,n", [(c, n) for c in (0, 1) for n in SIZES[c]])
def test_pairing_batches(gpu, curve, n):
    g1, g2, _, gt = pairs(curve)
    idx = np.arange(n) % NP
    assert np.array_equal(gpu.pairing(curve, g1[idx], g2[idx]), gt[idx])


@pytest.mark.parametrize("curve", [0, 1])
def test_pairing_from_device_memory(gpu, curve):
    g1, g2, _, gt = pairs(curve)
    d1, d2 = gpu.DeviceBuffer.from_numpy(g1[:3]), gpu.DeviceBuffer.from_numpy(g2[:3])
    out = gpu.DeviceBuffer(8 * 3 * gpu.gt_words(curve))
    gpu.pairing(curve, d1.ptr.value, d2.ptr.value, on_device=True, n=3, out=out.ptr.value)
    assert np.array_equal(out.to_numpy().reshape(3, -1), gt[:3])


@pytest.mark.parametrize("curve", [0, 1])
def test_pairing_is_bilinear(gpu, curve):
    """e(a P, b Q) = e(P, Q)^(a b), the power taken in the model"""
    P = model(curve)
    g1, g2, _, gt = pairs(curve)
    rng = pyref.splitmix64(5 + curve)
    a, b = pyref.rand_below(rng, P.C.r), pyref.rand_below(rng, P.C.r)
    sw = lambda x: np.array(P.C.fr_to_words(x), dtype=np.uint64)
    ap = gpu.point_to_affine(curve, 1, gpu.point_scale(curve, 1, sw(a), gpu.point_from_affine(curve, 1, g1[0])))
    bq = gpu.point_to_affine(curve, 2, gpu.point_scale(curve, 2, sw(b), gpu.point_from_affine(curve, 2, g2[0])))
    want = P.gt_to_words(P.pow(P.gt_from_words(gt[0]), a * b % P.C.r))
    assert np.array_equal(gpu.pairing(curve, ap, bq)[0], want)


@pytest.mark.parametrize("curve", [0, 1])
def test_identity_arguments_give_one_and_leave_neighbours_alone(gpu, curve):
    P = model(curve)
    g1, g2, _, gt = pairs(curve)
    n = WAVE[curve] + 2
    idx = np.arange(n) % NP
    a, b, want = g1[idx].copy(), g2[idx].copy(), gt[idx].copy()
    one = P.gt_to_words(P.one())
    a[1] = 0; b[3] = 0; a[n - 1] = 0; b[n - 1] = 0
    a[0, 12:] = 0                                   # y == 0 with any x is the identity
    for i in (0, 1, 3, n - 1):
        want[i] = one
    assert np.array_equal(gpu.pairing(curve, a, b), want)


@pytest.mark.parametrize("curve", [0, 1])
def test_malformed_points_are_refused(gpu, curve):
    g1, g2, _, _ = pairs(curve)
    q = model(curve).q
    for which in range(3):
        a, b = g1[:3].copy(), g2[:3].copy()
        if which == 0:
            a[1, 12] ^= np.uint64(1)                # off the curve
        elif which == 1:
            b[2, 0] ^= np.uint64(1)
        else:
            a[0, :12] = np.array([(q >> (64 * i)) & (2 ** 64 - 1) for i in range(12)], dtype=np.uint64)   # x = q: not canonical
        with pytest.raises(gpu.Mnt753Error):
            gpu.pairing(curve, a, b)


# ---- verification keys ------------------------------------------------------------------------------------------------
def elements(curve, tag):
    return np.fromfile(os.path.join(K.fixture_dir(curve, tag), "vk_elements.bin"), dtype="<u8").astype(np.uint64)


@pytest.mark.parametrize("fixture", K.FIXTURES, ids=K.fixture_id)
def test_verification_key_is_the_references(gpu, fixture):
    """gt() and serialize() of a key made from vk_elements.bin against the vk.txt the reference wrote, byte for byte"""
    curve, tag = fixture
    want = open(os.path.join(K.fixture_dir(curve, tag), "vk.txt"), "rb").read()
    vk = gpu.VerificationKey.from_elements(curve, elements(curve, tag))
    assert vk.num_inputs == 1
    assert vk.gt().astype("<u8").tobytes() == want[:8 * gpu.gt_words(curve)]
    assert vk.serialize() == want
    vk.close()


@pytest.mark.parametrize("curve", [0, 1])
def test_accumulate_vs_oracle(gpu, curve):
    """ABC[0] + x ABC[1] for x = 0, 1, r - 1 and random x, against the oracle's MSM and the host group law"""
    C = model(curve).C
    el = elements(curve, "cut21")
    abc = el[-48:].reshape(2, 24)
    vk = gpu.VerificationKey.from_elements(curve, el)
    rng = pyref.splitmix64(9 + curve)
    xs = [0, 1, C.r - 1] + [pyref.rand_below(rng, C.r) for _ in range(70)]
    inputs = np.array([C.fr_to_words(x) for x in xs], dtype=np.uint64)
    got = vk.accumulate(inputs.reshape(len(xs), 1, 12))
    first = gpu.point_from_affine(curve, 1, abc[0])
    for i in list(range(6)) + [len(xs) - 1]:
        s = O.msm(curve, 1, abc[1:], inputs[i:i + 1])
        want = gpu.point_to_affine(curve, 1, gpu.point_add(curve, 1, first, gpu.point_from_affine(curve, 1, s)))
        assert np.array_equal(got[i], want), i
    bad = inputs[:2].copy()
    bad[1] = np.array([(C.r >> (64 * i)) & (2 ** 64 - 1) for i in range(12)], dtype=np.uint64)
    with pytest.raises(gpu.Mnt753Error):
        vk.accumulate(bad.reshape(2, 1, 12))
    vk.close()


# ---- verification of batches --------------------------------------------------------------------------------------------
def g16(curve, name):
    return os.path.join(PR.GOLDEN, f"g16_mnt{4 if curve == 0 else 6}", name)


@functools.lru_cache(maxsize=None)
def g16_key_parts(curve):
    """alpha_g1, beta_g2 (keys.bin), delta_g2 and ABC (vk.txt), the proof and its input of the g16 fixture"""
    name = f"g16_mnt{4 if curve == 0 else 6}"
    w2 = 24 * (2 if curve == 0 else 3)
    alpha, beta = PR.alpha_beta_words(name)
    raw = open(g16(curve, "vk.txt"), "rb").read()
    pos = 8 * w2
    assert raw[pos:pos + 1] == b"0"
    delta = np.frombuffer(raw[pos + 1:pos + 1 + 8 * w2], dtype="<u8").astype(np.uint64)
    pos += 1 + 8 * w2
    abc0 = np.frombuffer(raw[pos + 1:pos + 193], dtype="<u8").astype(np.uint64)
    pos += 193
    assert raw[pos:pos + 9] == b"1\n1\n0\n1\n0"
    abc1 = np.frombuffer(raw[pos + 9:pos + 9 + 192], dtype="<u8").astype(np.uint64)
    assert np.array_equal(delta, PR.delta_words(name))
    proof = np.fromfile(g16(curve, "full.bin"), dtype="<u8").astype(np.uint64)
    inp = np.fromfile(g16(curve, "input.bin"), dtype="<u8", count=24).astype(np.uint64)[12:]
    return alpha, beta, delta, np.concatenate([abc0, abc1]), proof, inp


@functools.lru_cache(maxsize=None)
def proof_pool(curve):
    """NP valid proofs (A' = rho A, B' = rho^-1 B, C) of the fixture's statement, and the same with A' alone (invalid)"""
    from __graft_entry__ import load_package
    pkg = load_package()
    C = model(curve).C
    w2 = 24 * (2 if curve == 0 else 3)
    proof = g16_key_parts(curve)[4]
    A, B, Cp = proof[:24], proof[24:24 + w2], proof[24 + w2:]
    rng = pyref.splitmix64(33 + curve)
    sw = lambda x: np.array(C.fr_to_words(x), dtype=np.uint64)
    scale = lambda g, x, p: pkg.point_to_affine(curve, g, pkg.point_scale(curve, g, sw(x), pkg.point_from_affine(curve, g, p)))
    good, half = [proof.copy()], []
    for _ in range(NP - 1):
        rho = pyref.rand_below(rng, C.r - 1) + 1
        a2, b2 = scale(1, rho, A), scale(2, pow(rho, -1, C.r), B)
        good.append(np.concatenate([a2, b2, Cp]))
        half.append(np.concatenate([a2, B, Cp]))
    return np.stack(good), np.stack(half)


def build_batch(curve, n):
    """-> proofs [n, words], inputs [n, 12], the verdicts that hold by construction.  Invalid proofs sit in the first and the last
    slot of the first wave (the last one lies next to the idle lane on MNT6753) and in the last slot of the batch; malformed ones
    in slots 1 .. 9 of batches that have them."""
    C = model(curve).C
    w2 = 24 * (2 if curve == 0 else 3)
    good, half = proof_pool(curve)
    inp = g16_key_parts(curve)[5]
    idx = np.arange(n) % NP
    proofs, inputs, want = good[idx].copy(), np.tile(inp, (n, 1)), np.zeros(n, dtype=np.uint8)
    raw = lambda v: np.array([(v >> (64 * i)) & (2 ** 64 - 1) for i in range(12)], dtype=np.uint64)
    invalid = sorted({0, WAVE[curve] - 1, n - 1} & set(range(n))) if n > 1 else []
    for k, i in enumerate(invalid):
        if k % 3 == 0:
            proofs[i] = half[i % (NP - 1)]                               # A' = rho A alone
        elif k % 3 == 1:
            proofs[i, 24 + w2:] = proofs[i, :24]                         # C := A
        else:
            inputs[i] = np.array(C.fr_to_words((C.fr_from_words([int(v) for v in inp]) + 1) % C.r), dtype=np.uint64)   # a wrong input
        want[i] = 2
    if n >= 21:
        proofs[1, :24] = 0                                               # the identity as A
        proofs[2, 24 + w2 + 12] ^= np.uint64(1)                          # C off the curve
        proofs[3, 24:36] = raw(C.q)                                      # x.c0 of B = q: not canonical
        inputs[4] = raw(C.r)                                             # an input that is not below r
        proofs[5, 12:24] = raw(C.q)                                      # y of A = q
        proofs[6, 24 + w2 - 12:24 + w2] = raw(C.q + 1)                   # the last component of B.y: another lane's flag
        proofs[7, 24 + w2:36 + w2] = raw(C.q)                            # x of C = q
        proofs[8, 24 + 12] ^= np.uint64(1)                               # B off the twist
        proofs[9, 24 + w2 // 2:24 + w2] = 0                              # the identity as B
        want[1:10] = 1
    return proofs, inputs, want


@pytest.mark.parametrize("curve", [0, 1])
def test_the_fixture_proof_verifies_and_another_delta_rejects(gpu, curve):
    alpha, beta, delta, abc, proof, inp = g16_key_parts(curve)
    vk = gpu.VerificationKey(curve, alpha, beta, delta, abc)
    assert np.array_equal(vk.gt(), PR.vk_head(f"g16_mnt{4 if curve == 0 else 6}"))
    assert list(vk.verify(proof, inp)) == [0]
    good, _ = proof_pool(curve)
    assert list(vk.verify(good[:2], np.tile(inp, (2, 1)))) == [0, 0]
    vk.close()
    other = gpu.VerificationKey(curve, alpha, beta, beta, abc)           # a key with another delta
    assert list(other.verify(good[:2], np.tile(inp, (2, 1)))) == [2, 2]
    other.close()


@pytest.mark.parametrize("curve,n", [(c, n) for c in (0, 1) for n in SIZES[c]])
def test_verify_batches(gpu, curve, n):
    alpha, beta, delta, abc, _, _ = g16_key_parts(curve)
    vk = gpu.VerificationKey(curve, alpha, beta, delta, abc)
    proofs, inputs, want = build_batch(curve, n)
    assert list(vk.verify(proofs, inputs)) == list(want)
    assert vk.coefficient_bytes() == 2 * (4 * 376 + 2 * (174 + (1 if curve == 0 else 0))) * (2, 3)[curve] * 112
    if n == SIZES[curve][3]:                                             # the same under a workspace cap of 5 proofs per chunk
        vk.set_workspace_cap(5 * (194 + 96 + 8 * proofs.shape[1] + 96))
        assert list(vk.verify(proofs, inputs)) == list(want)
        vk.set_workspace_cap(1)                                          # below one proof: chunks of one
        assert list(vk.verify(proofs[:3], inputs[:3])) == list(want[:3])
        vk.set_workspace_cap(0)
    if n == SIZES[curve][2]:                                             # the same from device memory
        dp, di = gpu.DeviceBuffer.from_numpy(proofs), gpu.DeviceBuffer.from_numpy(inputs)
        assert list(vk.verify(dp.ptr.value, di.ptr.value, on_device=True, n=n)) == list(want)
    vk.close()


# ---- the command line -------------------------------------------------------------------------------------------------------
from test_groth16_cpu import EXE, NAME, REF  # noqa: E402


def cli(args):
    import subprocess
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True)


def cli_proof(curve, tmp_path, names=("good", "other")):
    """main_hip generate (the fixture's randomness, and the same with delta := t) -> compute-r1cs -> complete with the first key
    -> the key directories and the proof"""
    fdir = K.fixture_dir(curve, "cut21")
    f = lambda name: os.path.join(fdir, name)
    rnd = np.fromfile(f("randomness.bin"), dtype="<u8")
    other = rnd.copy(); other[36:48] = rnd[0:12]                       # delta := t
    (tmp_path / "other.bin").write_bytes(other.tobytes())
    outs = {}
    for name in names:
        out = tmp_path / name
        rand = f("randomness.bin") if name == "good" else tmp_path / "other.bin"
        assert cli([NAME[curve], "generate", f("r1cs_in.bin"), out, "--randomness", rand, "--quiet"]).returncode == 0
        outs[name] = out
    out = outs["good"]
    chal, full = out / "challenge.bin", out / "full.bin"
    r = cli([NAME[curve], "compute-r1cs", out / "params.bin", out / "r1cs.bin", f("witness.bin"), chal])
    assert r.returncode == 0, r.stderr
    r = cli([NAME[curve], "complete", out / "keys.bin", f("witness.bin"), chal, full, "--s-seed", "99"])
    assert r.returncode == 0, r.stderr
    return outs, full, f


@pytest.mark.parametrize("curve", [0, 1])
def test_generate_prove_verify_on_the_command_line(gpu, curve, tmp_path):
    """main_hip generate -> compute-r1cs -> complete -> verify prints VERIFIED for the key's own proof and REJECTED (exit 3) against
    the key made with another delta; `main_hip vk` writes the reference's vk.txt.  `verify` goes through B::verify."""
    outs, full, f = cli_proof(curve, tmp_path)
    out = outs["good"]
    r = cli([NAME[curve], "verify", out / "vk_elements.bin", f("witness.bin"), full, full])
    assert (r.returncode, r.stdout.split()) == (0, ["VERIFIED", "VERIFIED"]), r.stdout + r.stderr
    r = cli([NAME[curve], "verify", outs["other"] / "vk_elements.bin", f("input.bin"), full])
    assert (r.returncode, r.stdout.split()) == (3, ["REJECTED"]), r.stdout + r.stderr
    r = cli([NAME[curve], "verify", out / "vk_elements.bin", f("r1cs.bin"), full])          # a file that does not start with 1
    assert r.returncode == 3 and "constant 1" in r.stderr and r.stdout == ""
    r = cli([NAME[curve], "vk", out / "vk_elements.bin", tmp_path / "vk.txt"])
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "vk.txt").read_bytes() == open(f("vk.txt"), "rb").read()
    # the same proof through the Python objects: GeneratedKey.verification_key()
    el = np.fromfile(out / "vk_elements.bin", dtype="<u8").astype(np.uint64)
    w2 = gpu.affine_words(curve, 2)
    singles = {"alpha_g1": el[:24], "beta_g2": el[24:24 + w2], "delta_g2": el[24 + w2:24 + 2 * w2]}
    queries = {k: (el[24 + 2 * w2:] if k == "ABC" else np.zeros(0, dtype=np.uint64)) for k, _ in gpu.GeneratedKey.QUERIES}
    vk = gpu.GeneratedKey.from_host(curve, 1, 0, 0, 0, queries, singles, None).verification_key()
    assert vk.serialize() == open(f("vk.txt"), "rb").read()
    inp = np.fromfile(f("input.bin"), dtype="<u8", count=24).astype(np.uint64)[12:]
    assert list(vk.verify(np.fromfile(full, dtype="<u8").astype(np.uint64), inp)) == [0]
    vk.close()


@pytest.mark.parametrize("curve", [0, 1])
def test_the_reference_verifier_accepts_against_a_device_written_key(gpu, curve, tmp_path):
    """The reference's verifier accepts the device-made proof of the scenario above against a DEVICE-WRITTEN vk.txt (`main_hip vk`),
    placed in a directory of its own beside input.bin.  Needs the reference build (oracle/_ref/ref_groth16): looked for first."""
    import shutil
    import subprocess
    ref = O.need_ref("ref_groth16")
    outs, full, f = cli_proof(curve, tmp_path, names=("good",))
    vdir = tmp_path / "refdir"
    vdir.mkdir()
    r = cli([NAME[curve], "vk", outs["good"] / "vk_elements.bin", vdir / "vk.txt"])
    assert r.returncode == 0, r.stderr
    shutil.copy(f("input.bin"), vdir / "input.bin")
    v = subprocess.run([ref, "verify", NAME[curve], str(vdir), str(full)], capture_output=True, text=True)
    assert v.returncode == 0 and v.stdout.strip().splitlines()[-1] == "VERIFIED", v.stdout + v.stderr


@pytest.mark.parametrize("curve", [0, 1])
def test_wrapper_class_pairing_and_verify(gpu, curve, tmp_path):
    """B::pairing and B::verify of include/prover_hip_functions.hpp from a C++ caller (tools/host_tests/pairing_wrapper_test.cpp, built
    by make): the GT element of the g16 fixture's key, its proof accepted, the proof with C := A rejected"""
    import subprocess
    exe = os.path.join(O.ROOT, "snark-challenge-prover-reference_amd", "pairing_wrapper_test")
    r = subprocess.run([exe, NAME[curve], g16(curve, "keys.bin"), g16(curve, "vk.txt"), str(g16_elements_file(curve, tmp_path)), g16(curve, "input.bin"),
                        g16(curve, "full.bin")], capture_output=True, text=True)
    assert r.returncode == 0 and "wrapper pairing OK" in r.stdout, r.stdout + r.stderr


def g16_elements_file(curve, tmp_path):
    """alpha_g1 | beta_g2 | delta_g2 | ABC_g1 of the g16 fixture, as `generate` would write them"""
    alpha, beta, delta, abc, _, _ = g16_key_parts(curve)
    path = tmp_path / "vk_elements.bin"
    path.write_bytes(np.concatenate([alpha, beta, delta, abc]).astype("<u8").tobytes())
    return path
