"""GPU: folded Groth16 verification (mnt753_groth16_verify_folded) against the Python-integer model of
tests/fold_ref.py.  Every comparison is of all words; there is no tolerance.

Shapes: one lane group per proof -- g = 32 groups per wave and 128 per workgroup on MNT4753, 21 and 84 on MNT6753 (lane 63 idles).
The batches are 1, 2, a full wave, a wave and one, a workgroup and one, and two workgroups and one (257 / 169: the second-level
product then has three partial products, one of them from a single lane group).  Batches cycle the 7 valid proofs of
test_pairing_gpu.proof_pool; the coefficients are fixed 128-bit values, distinct per proof."""
import functools
import subprocess

import numpy as np
import pytest

import fold_ref as FR
import pyref
import subgroup_ref as S
import test_pairing_gpu as TP
import test_subgroup_gpu as TS
from test_groth16_cpu import EXE, NAME

pytestmark = pytest.mark.gpu

G = S.GROUPS_PER_WAVE
SIZES = {c: [1, 2, G[c], G[c] + 1, 4 * G[c] + 1, 8 * G[c] + 1] for c in (0, 1)}
EDGE_SIZES = {c: [G[c] + 1, 8 * G[c] + 1] for c in (0, 1)}
W2 = TS.W2


def rhos(n, seed=7):
    """n distinct coefficients in [1, 2^128): the first has its top bit set, the second is 1, the third 2^127 + 1"""
    rng = pyref.splitmix64(seed)
    out = [(1 << 127) | pyref.rand_below(rng, 1 << 127), 1, (1 << 127) + 1]
    while len(out) < n:
        out.append(pyref.rand_below(rng, (1 << 128) - 1) + 1)
    return out[:n]


_KEYS = {}


def key(gpu, curve):
    if curve not in _KEYS:
        alpha, beta, delta, abc, _, _ = TP.g16_key_parts(curve)
        _KEYS[curve] = gpu.VerificationKey(curve, alpha, beta, delta, abc)
    return _KEYS[curve]


def valid_batch(curve, n):
    good, _ = TP.proof_pool(curve)
    inp = TP.g16_key_parts(curve)[5]
    return good[np.arange(n) % TP.NP].copy(), np.tile(inp, (n, 1))


def model_batch(curve, proofs, inputs):
    C = FR.model(curve).C
    return [FR.proof_from_words(curve, p) for p in proofs], [[C.fr_from_words([int(v) for v in row[12 * j:12 * j + 12]]) for j in range(len(row) // 12)] for row in inputs]


def edge_positions(curve, n):
    """index 0, the last group of the first wave, n - 1"""
    return sorted({0, G[curve] - 1, n - 1} & set(range(n)))


@pytest.mark.parametrize("curve,n", [(c, n) for c in (0, 1) for n in (1, 3)])
def test_parts_vs_reference(gpu, curve, n):
    """F (the unreduced product), S, T and rho of the hook are the model's words"""
    P = FR.model(curve)
    proofs, inputs = valid_batch(curve, n)
    k = rhos(n)
    want = FR.parts(FR.g16_key(curve), *model_batch(curve, proofs, inputs), k)
    got = key(gpu, curve).test_fold_parts(proofs, inputs, k)
    assert np.array_equal(got["rho"], FR.fr_words(curve, want["rho"]))
    assert np.array_equal(got["t"], FR.g1_words(curve, want["T"]))
    assert np.array_equal(got["s"], FR.g1_words(curve, want["S"]))
    assert np.array_equal(got["f"], P.gt_to_words(want["F"]))
    assert got["accepted"] and not got["status"].any() and FR.verdict(FR.g16_key(curve), want)


@pytest.mark.parametrize("curve,n", [(c, n) for c in (0, 1) for n in EDGE_SIZES[c]])
def test_reduction_at_the_edges(gpu, curve, n):
    """F against the Python tower product of the per-pair unreduced Miller values, which come from the test_miller_loop hook on the
    model's U_i and the proofs' B_i (code from before the fold, pinned against pairing_ref by test_pairing_gpu); T against the model's sum"""
    P = FR.model(curve)
    proofs, inputs = valid_batch(curve, n)
    k = rhos(n)
    U, T, Sp, rho, _ = FR.g1_parts(FR.g16_key(curve), *model_batch(curve, proofs, inputs), k)
    uw = np.stack([FR.g1_words(curve, u) for u in U])
    per_pair = gpu.api.test_miller_loop(curve, 1, uw, proofs[:, 24:24 + W2[curve]])
    want_f = FR.product(curve, [P.gt_from_words(w) for w in per_pair])
    got = key(gpu, curve).test_fold_parts(proofs, inputs, k)
    assert np.array_equal(got["f"], P.gt_to_words(want_f))
    assert np.array_equal(got["t"], FR.g1_words(curve, T))
    assert np.array_equal(got["s"], FR.g1_words(curve, Sp))
    assert np.array_equal(got["rho"], FR.fr_words(curve, rho))
    assert got["accepted"] and not got["status"].any()


@pytest.mark.parametrize("curve,n", [(c, n) for c in (0, 1) for n in SIZES[c]])
def test_verdicts(gpu, curve, n):
    """a valid batch is accepted with an all-zero status; one tampered C (C := A: on the curve, wrong) at index 0, in the last group of
    the first wave or at n - 1 rejects it, and the status stays zero: the fold does not name the proof"""
    vk = key(gpu, curve)
    proofs, inputs = valid_batch(curve, n)
    k = rhos(n)
    accepted, status = vk.verify_folded(proofs, inputs, k)
    assert accepted and status.shape == (n,) and not status.any()
    for i in edge_positions(curve, n):
        bent = proofs.copy()
        bent[i, 24 + W2[curve]:] = bent[i, :24]
        accepted, status = vk.verify_folded(bent, inputs, k)
        assert not accepted and not status.any(), (n, i)
    if n == G[curve] + 1:                                                    # from device memory, with coefficients as words
        dp, di = gpu.DeviceBuffer.from_numpy(proofs), gpu.DeviceBuffer.from_numpy(inputs)
        accepted, status = vk.verify_folded(dp.ptr.value, di.ptr.value, FR.coefficient_words(k), on_device=True, n=n)
        assert accepted and not status.any()
        wrong = inputs.copy()
        wrong[n - 1] = np.array(FR.model(curve).C.fr_to_words(12345), dtype=np.uint64)   # a wrong public input for the last proof
        accepted, status = vk.verify_folded(proofs, wrong, k)
        assert not accepted and not status.any()


@pytest.mark.parametrize("curve", [0, 1])
def test_status_bytes(gpu, curve):
    """B outside G2 (lifted twist points, and B + [r] P) gives 3, an A off the curve gives 1, at index 0, in the last group of the
    first wave, in the first of the next and at n - 1; the neighbours stay 0 and the batch is rejected"""
    n = 4 * G[curve] + 1
    vk = key(gpu, curve)
    proofs, inputs = valid_batch(curve, n)
    want = np.zeros(n, dtype=np.uint8)
    for j, i in enumerate(TS.edges(curve, n)):
        proofs[i, 24:24 + W2[curve]] = TS.bad_b(curve)[j % 3]
        want[i] = 3
    accepted, status = vk.verify_folded(proofs, inputs, rhos(n))
    assert not accepted and list(status) == list(want)
    proofs, inputs = valid_batch(curve, n)
    want = np.zeros(n, dtype=np.uint8)
    for i in TS.edges(curve, n):
        proofs[i, 12] ^= np.uint64(1)                                        # y of A: off the curve
        want[i] = 1
    proofs[2, 24 + W2[curve] // 2:24 + W2[curve]] = 0                        # the identity as B
    proofs[3, 24 + W2[curve]:36 + W2[curve]] = TS.raw(FR.model(curve).C.q)   # x of C = q: not canonical
    inputs[4] = TS.raw(FR.model(curve).C.r)                                  # an input that is not below r
    proofs[5, 24:24 + W2[curve]] = TS.bad_b(curve)[1]
    want[2:5] = 1
    want[5] = 3
    accepted, status = vk.verify_folded(proofs, inputs, rhos(n))
    assert not accepted and list(status) == list(want)
    assert list(vk.verify(proofs, inputs, check_subgroup=True)) == list(want)    # (these cases carry the same byte per proof)


def bent_pair(curve):
    """the first two proofs of the pool with C_0 + D and C_1 - D"""
    C = FR.model(curve).C
    proofs, inputs = valid_batch(curve, 2)
    p = [FR.proof_from_words(curve, w) for w in proofs]
    D = C.mul(0xD15EA5E, C.gen(1), 1)
    bent = [(p[0][0], p[0][1], C.add(p[0][2], D, 1)), (p[1][0], p[1][1], C.add(p[1][2], C.neg(D), 1))]
    return np.stack([FR.proof_to_words(curve, b) for b in bent]), inputs


@pytest.mark.parametrize("curve", [0, 1])
def test_cancelling_pair(gpu, curve):
    """two wrong proofs whose defects cancel: with rho = (1, 1) the fold accepts what the per-proof verifier rejects twice; with
    rho = (1, 2) it rejects.  The reason the coefficients must be unpredictable -- and the coefficients are applied."""
    vk = key(gpu, curve)
    proofs, inputs = bent_pair(curve)
    assert list(vk.verify(proofs, inputs)) == [2, 2]
    assert vk.verify_folded(proofs, inputs, [1, 1])[0] is True
    assert vk.verify_folded(proofs, inputs, [1, 2])[0] is False
    assert list(vk.verify(proofs, inputs, fold=True)) == [2, 2]              # (random coefficients: 2^-128 to pass)


@pytest.mark.parametrize("curve", [0, 1])
def test_two_public_inputs(gpu, curve):
    """No committed key has more than one public input.  A key with ABC = (ABC_0, ABC_1, ABC_1) and the inputs (x - s_i, s_i), s_i
    different per proof, accumulates to the fixture's point, so the pool's proofs stay valid: the column reduction runs with two
    columns of inputs that differ per proof, S is the model's, the batch is accepted, and one changed input rejects it."""
    C = FR.model(curve).C
    alpha, beta, delta, abc, _, inp = TP.g16_key_parts(curve)
    n = G[curve] + 2
    proofs, _ = valid_batch(curve, n)
    x = C.fr_from_words([int(v) for v in inp])
    rng = pyref.splitmix64(41 + curve)
    split = [pyref.rand_below(rng, C.r) for _ in range(n)]
    xs = [[(x - s) % C.r, s] for s in split]
    inputs = np.array([C.fr_to_words(a) + C.fr_to_words(b) for a, b in xs], dtype=np.uint64)
    vk = gpu.VerificationKey(curve, alpha, beta, delta, np.concatenate([abc, abc[24:]]))
    assert vk.num_inputs == 2
    k = rhos(n)
    g16 = FR.g16_key(curve)
    mkey = FR.Key(curve, g16.alpha_beta, g16.delta, g16.abc + [g16.abc[1]])
    _, T, Sp, rho, c = FR.g1_parts(mkey, [FR.proof_from_words(curve, p) for p in proofs], xs, k)
    assert c[0] != c[1]
    got = vk.test_fold_parts(proofs, inputs, k)
    assert np.array_equal(got["s"], FR.g1_words(curve, Sp)) and np.array_equal(got["t"], FR.g1_words(curve, T))
    assert got["accepted"] and not got["status"].any()
    assert list(vk.verify(proofs[:3], inputs[:3])) == [0, 0, 0]
    inputs[n - 1, 12:] = np.array(C.fr_to_words((split[n - 1] + 1) % C.r), dtype=np.uint64)
    accepted, status = vk.verify_folded(proofs, inputs, k)
    assert not accepted and not status.any()
    vk.set_workspace_cap(7 * (546 + 96 * 3 + 8 * proofs.shape[1] + 96 * 2))  # the same in chunks of 7: the columns of every chunk
    inputs[n - 1, 12:] = np.array(C.fr_to_words(split[n - 1]), dtype=np.uint64)
    again = vk.test_fold_parts(proofs, inputs, k)
    assert again["accepted"] and all(np.array_equal(again[f], got[f]) for f in ("f", "s", "t", "rho"))
    vk.close()


@pytest.mark.parametrize("curve", [0, 1])
def test_chunks_give_the_same_parts(gpu, curve):
    """a workspace cap of 8 proofs per chunk at n = 33 / 22 (5 / 3 chunks): F, T, S, rho and the verdict are those of one chunk, for a
    valid batch and for one with a tampered C in the last chunk"""
    n = G[curve] + 1
    proofs, inputs = valid_batch(curve, n)
    k = rhos(n)
    alpha, beta, delta, abc, _, _ = TP.g16_key_parts(curve)
    vk = gpu.VerificationKey(curve, alpha, beta, delta, abc)
    for bend in (False, True):
        if bend:
            proofs[n - 1, 24 + W2[curve]:] = proofs[n - 1, :24]
        vk.set_workspace_cap(0)
        whole = vk.test_fold_parts(proofs, inputs, k)
        vk.set_workspace_cap(8 * (546 + 96 * 2 + 8 * proofs.shape[1] + 96))
        pieces = vk.test_fold_parts(proofs, inputs, k)
        assert all(np.array_equal(pieces[f], whole[f]) for f in ("f", "s", "t", "rho", "status"))
        assert pieces["accepted"] == whole["accepted"] == (not bend)
    vk.set_workspace_cap(1)                                                  # below one proof: chunks of one
    ones = vk.test_fold_parts(proofs[:3], inputs[:3], k[:3])
    vk.set_workspace_cap(0)
    assert all(np.array_equal(ones[f], vk.test_fold_parts(proofs[:3], inputs[:3], k[:3])[f]) for f in ("f", "s", "t", "rho"))
    vk.close()


@pytest.mark.parametrize("curve", [0, 1])
def test_errors_and_the_empty_batch(gpu, curve):
    vk = key(gpu, curve)
    proofs, inputs = valid_batch(curve, 3)
    with pytest.raises(gpu.Mnt753Error, match="coefficient is zero"):
        vk.verify_folded(proofs, inputs, [5, 0, 7])
    with pytest.raises(gpu.Mnt753Error):
        vk.verify_folded(proofs, inputs, [5, 7])                             # one coefficient per proof
    accepted, status = vk.verify_folded(np.zeros((0, proofs.shape[1]), dtype=np.uint64), np.zeros((0, 12), dtype=np.uint64), [], n=0)
    assert accepted and status.size == 0
    accepted, status = vk.verify_folded(proofs, inputs)                      # coefficients drawn by the wrapper
    assert accepted and not status.any()


@pytest.mark.parametrize("curve", [0, 1])
def test_verify_with_fold_falls_back_to_the_per_proof_pass(gpu, curve):
    vk = key(gpu, curve)
    n = G[curve] + 1
    proofs, inputs = valid_batch(curve, n)
    assert list(vk.verify(proofs, inputs, fold=True)) == [0] * n
    proofs[n - 2, 24 + W2[curve]:] = proofs[n - 2, :24]
    want = vk.verify(proofs, inputs, check_subgroup=True)
    assert list(want) == [0] * (n - 2) + [2, 0]
    assert list(vk.verify(proofs, inputs, fold=True)) == list(want)
    proofs[1, 24:24 + W2[curve]] = TS.bad_b(curve)[0]
    assert list(vk.verify(proofs, inputs, fold=True)) == list(vk.verify(proofs, inputs, check_subgroup=True)) == [0, 3] + [0] * (n - 4) + [2, 0]


@pytest.mark.parametrize("curve", [0, 1])
def test_cli_fold(gpu, curve, tmp_path):
    """main_hip verify --fold --fold-coefficients: the fixture's proof (twice) is accepted in one line, exit 0; with a tampered copy the
    per-proof lines follow, exit 3; a coefficient file of the wrong size is refused"""
    el = TP.g16_elements_file(curve, tmp_path)
    inp, full = TP.g16(curve, "input.bin"), TP.g16(curve, "full.bin")
    proof = np.fromfile(full, dtype="<u8")
    proof[24 + W2[curve]:] = proof[:24]
    bent = tmp_path / "bent.bin"
    proof.astype("<u8").tofile(bent)
    coef = tmp_path / "coef.bin"
    FR.coefficient_words(rhos(2)).astype("<u8").tofile(coef)
    cli = lambda args: subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True)
    r = cli([NAME[curve], "verify", el, inp, full, full, "--fold", "--fold-coefficients", coef])
    assert (r.returncode, r.stdout.splitlines()) == (0, ["VERIFIED 2 proofs (folded)"]), r.stdout + r.stderr
    r = cli([NAME[curve], "verify", el, inp, full, "--fold"])
    assert (r.returncode, r.stdout.splitlines()) == (0, ["VERIFIED 1 proofs (folded)"]), r.stdout + r.stderr
    r = cli([NAME[curve], "verify", el, inp, full, bent, "--fold", "--fold-coefficients", coef])
    assert (r.returncode, r.stdout.splitlines()) == (3, ["VERIFIED", "REJECTED"]), r.stdout + r.stderr
    r = cli([NAME[curve], "verify", el, inp, full, "--fold", "--fold-coefficients", coef])
    assert r.returncode == 1 and r.stdout == "" and "one 128-bit coefficient per proof" in r.stderr
