"""GPU: the folded verification with one tail per segment (mnt753_groth16_verify_folded_locate).  The
references are code from before this call: the fold's own hook test_fold_parts on the proofs of ONE segment (F_s, S_s, T_s, rho_s word
for word) and the per-proof verifier with the subgroup check (the verdict bytes).  Every comparison is of all words or bytes; there
is no tolerance.

Shapes: g = fold_segment_proofs(curve) = 128 / 84 proofs per segment, one workgroup of the Miller kernel.  Batches are 1, 2, g, g + 1
(a full segment and a segment of one proof) and 2 g + 1 (three segments: the tails of one wave then run three different segments);
tampered proofs sit at 0, g - 1, g and n - 1, the two sides of a boundary and the ends."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import fold_ref as FR
import pyref
import test_fold_gpu as TF
import test_pairing_gpu as TP
import test_subgroup_gpu as TS
from test_groth16_cpu import EXE, NAME

pytestmark = pytest.mark.gpu

W2 = TS.W2
EINVAL = -1
TB = {0: 448, 1: 672}                                                        # bytes of one GT element in device form


def seg(gpu, curve):
    return gpu.fold_segment_proofs(curve)


def bend(proofs, curve, i):
    """C := A at proof i: on the curve, wrong"""
    proofs[i, 24 + W2[curve]:] = proofs[i, :24]


def segment_of(i, g):
    return i // g


def segment_sizes(n, g):
    return [min(g, n - a) for a in range(0, n, g)]


@pytest.mark.parametrize("curve,k", [(c, k) for c in (0, 1) for k in (1, 2)])
def test_parts_are_the_folds_parts_of_every_segment(gpu, curve, k):
    """n = k g + 1: F_s, S_s, T_s, rho_s of every segment are the words the EXISTING hook gives for that segment's proofs alone"""
    g = seg(gpu, curve)
    n = k * g + 1
    vk = TF.key(gpu, curve)
    proofs, inputs = TF.valid_batch(curve, n)
    rho = TF.rhos(n)
    got = vk.test_fold_segment_parts(proofs, inputs, rho)
    assert got["report"]["segments"] == -(-n // g) == k + 1 and got["f"].shape[0] == k + 1
    for s in range(k + 1):
        a, b = s * g, min(n, (s + 1) * g)
        want = vk.test_fold_parts(proofs[a:b], inputs[a:b], rho[a:b])
        for part in ("f", "s", "t", "rho"):
            assert np.array_equal(got[part][s], want[part]), (s, part)
        assert got["accepted"][s] == 1 and want["accepted"]
    assert not got["status"].any() and not got["verdicts"].any()
    assert got["report"]["segments_rejected"] == 0 and got["report"]["proofs_rechecked"] == 0


@pytest.mark.parametrize("curve", [0, 1])
def test_a_valid_batch_is_accepted_without_a_recheck(gpu, curve):
    g = seg(gpu, curve)
    vk = TF.key(gpu, curve)
    for n in (1, 2, g, g + 1, 2 * g + 1):
        proofs, inputs = TF.valid_batch(curve, n)
        verdicts, rep = vk.verify_folded_locate(proofs, inputs, TF.rhos(n))
        assert verdicts.shape == (n,) and not verdicts.any(), n
        assert (rep["segments"], rep["segments_rejected"], rep["proofs_rechecked"]) == (-(-n // g), 0, 0), n


@pytest.mark.parametrize("curve,k", [(c, k) for c in (0, 1) for k in (1, 2)])
def test_one_wrong_proof_costs_one_segment(gpu, curve, k):
    """C := A at 0, g - 1, g or n - 1: the verdicts are the per-proof verifier's, byte for byte, and ONE segment was rechecked -- an
    implementation that rechecks everything fails the count"""
    g = seg(gpu, curve)
    n = k * g + 1
    vk = TF.key(gpu, curve)
    good, inputs = TF.valid_batch(curve, n)
    rho = TF.rhos(n)
    sizes = segment_sizes(n, g)
    for i in (0, g - 1, g, n - 1):
        proofs = good.copy()
        bend(proofs, curve, i)
        verdicts, rep = vk.verify_folded_locate(proofs, inputs, rho)
        want = vk.verify(proofs, inputs, check_subgroup=True)
        assert list(want) == [2 if j == i else 0 for j in range(n)]
        assert list(verdicts) == list(want), i
        assert rep["segments_rejected"] == 1 and rep["proofs_rechecked"] == sizes[segment_of(i, g)], (i, rep)


@pytest.mark.parametrize("curve", [0, 1])
def test_status_bytes(gpu, curve):
    """test_fold_gpu.test_status_bytes's designed batch at n = 2 g + 1 -- an A off the curve at TS.edges, the identity as B, a
    non-canonical x of C, an input >= r, a B outside G2 -- with one C := A in a segment that also holds malformed proofs; then one
    more in the segment that holds none.  The verdicts are the per-proof verifier's and the rejected segments are the touched ones."""
    g = seg(gpu, curve)
    n = 2 * g + 1
    vk = TF.key(gpu, curve)
    proofs, inputs = TF.valid_batch(curve, n)
    touched = set()
    for i in TS.edges(curve, n):
        proofs[i, 12] ^= np.uint64(1)                                        # y of A: off the curve
        touched.add(segment_of(i, g))
    proofs[2, 24 + W2[curve] // 2:24 + W2[curve]] = 0                        # the identity as B
    proofs[3, 24 + W2[curve]:36 + W2[curve]] = TS.raw(FR.model(curve).C.q)   # x of C = q: not canonical
    inputs[4] = TS.raw(FR.model(curve).C.r)                                  # an input that is not below r
    proofs[5, 24:24 + W2[curve]] = TS.bad_b(curve)[1]                        # B outside G2
    bend(proofs, curve, 10)                                                  # beside malformed proofs
    touched.add(0)
    assert touched == {0, 2}
    sizes = segment_sizes(n, g)
    rho = TF.rhos(n)
    for extra in (None, g + 3):
        if extra is not None:
            bend(proofs, curve, extra)                                       # in the segment that held no flagged proof
            touched.add(segment_of(extra, g))
        want = vk.verify(proofs, inputs, check_subgroup=True)
        assert want[10] == 2 and want[5] == 3 and list(want[2:5]) == [1, 1, 1] and want[n - 1] == 1
        verdicts, rep = vk.verify_folded_locate(proofs, inputs, rho)
        assert list(verdicts) == list(want), extra
        assert rep["segments_rejected"] == len(touched) and rep["proofs_rechecked"] == sum(sizes[s] for s in touched), (extra, rep)


@pytest.mark.parametrize("curve", [0, 1])
def test_the_boundary_is_where_the_call_says_it_is(gpu, curve):
    """the cancelling pair with rho = (1, 1): inside one segment it is accepted -- the documented limit of predictable coefficients --
    and across the boundary (g - 1, g) both proofs get 2 and two segments are rejected"""
    g = seg(gpu, curve)
    n = g + 1
    vk = TF.key(gpu, curve)
    pair, _ = TF.bent_pair(curve)
    for at, want, rejected in ((0, [0] * n, 0), (g - 1, [0] * (g - 1) + [2, 2], 2)):
        proofs, inputs = TF.valid_batch(curve, n)
        rho = TF.rhos(n)
        proofs[at], proofs[at + 1] = pair[0], pair[1]
        rho[at] = rho[at + 1] = 1
        verdicts, rep = vk.verify_folded_locate(proofs, inputs, rho)
        assert list(verdicts) == want, at
        assert rep["segments_rejected"] == rejected and rep["proofs_rechecked"] == (n if rejected else 0)
    assert list(vk.verify(pair, TF.valid_batch(curve, 2)[1])) == [2, 2]


@pytest.mark.parametrize("curve", [0, 1])
def test_a_wrong_public_input(gpu, curve):
    g = seg(gpu, curve)
    n = g + 1
    vk = TF.key(gpu, curve)
    proofs, inputs = TF.valid_batch(curve, n)
    inputs[n - 1] = np.array(FR.model(curve).C.fr_to_words(12345), dtype=np.uint64)
    verdicts, rep = vk.verify_folded_locate(proofs, inputs, TF.rhos(n))
    assert list(verdicts) == [0] * (n - 1) + [2]
    assert rep["segments_rejected"] == 1 and rep["proofs_rechecked"] == 1


@pytest.mark.parametrize("curve", [0, 1])
def test_two_public_inputs_unprepared_and_prepared(gpu, curve):
    """test_fold_gpu.test_two_public_inputs's key, ABC = (ABC_0, ABC_1, ABC_1) with the inputs (x - s_i, s_i), at n = g + 1 with one
    wrong input row: S_s of the device ladder (the key as it is) and of the walk over the input tables (prepare_inputs) are the same
    words, and the fold's own S for the segment; the verdicts are the same"""
    Cm = FR.model(curve).C
    g = seg(gpu, curve)
    n = g + 1
    alpha, beta, delta, abc, _, inp = TP.g16_key_parts(curve)
    proofs, _ = TF.valid_batch(curve, n)
    x = Cm.fr_from_words([int(v) for v in inp])
    rng = pyref.splitmix64(43 + curve)
    split = [pyref.rand_below(rng, Cm.r) for _ in range(n)]
    inputs = np.array([Cm.fr_to_words((x - s) % Cm.r) + Cm.fr_to_words(s) for s in split], dtype=np.uint64)
    inputs[3, 12:] = np.array(Cm.fr_to_words((split[3] + 1) % Cm.r), dtype=np.uint64)      # one wrong row, in segment 0
    rho = TF.rhos(n)
    vk = gpu.VerificationKey(curve, alpha, beta, delta, np.concatenate([abc, abc[24:]]))
    assert vk.num_inputs == 2
    plain = vk.test_fold_segment_parts(proofs, inputs, rho)
    want = vk.test_fold_parts(proofs[:g], inputs[:g], rho[:g])
    assert np.array_equal(plain["s"][0], want["s"]) and np.array_equal(plain["t"][0], want["t"]) and np.array_equal(plain["f"][0], want["f"])
    assert list(plain["verdicts"]) == [0, 0, 0, 2] + [0] * (n - 4) and list(plain["accepted"]) == [0, 1]
    assert plain["report"]["segments_rejected"] == 1 and plain["report"]["proofs_rechecked"] == g
    vk.prepare_inputs()
    tables = vk.test_fold_segment_parts(proofs, inputs, rho)
    for part in ("f", "s", "t", "rho", "accepted", "status", "verdicts"):
        assert np.array_equal(tables[part], plain[part]), part
    verdicts, rep = vk.verify_folded_locate(proofs, inputs, rho)
    assert list(verdicts) == list(plain["verdicts"]) and rep["proofs_rechecked"] == g
    vk.close()


@pytest.mark.parametrize("curve", [0, 1])
def test_chunks_are_whole_segments(gpu, curve):
    """n = 2 g + 1 (three segments) under a cap that leaves exactly one segment's proofs per chunk, two segments', and less than one
    (still one segment per chunk): the call runs 3, 2 and 3 chunks, 1 without a cap, and the verdicts and every segment's parts are
    those of the call without a cap"""
    g = seg(gpu, curve)
    n = 2 * g + 1
    proofs, inputs = TF.valid_batch(curve, n)
    bend(proofs, curve, g)
    rho = TF.rhos(n)
    alpha, beta, delta, abc, _, _ = TP.g16_key_parts(curve)
    vk = gpu.VerificationKey(curve, alpha, beta, delta, abc)
    # a host batch with one public input: per proof of a chunk 546 + 96 (1 + 1) and its staged copy; per segment of the call
    # 516 + g + 96 (1 + 1) + one GT element, which comes off the cap first
    per_proof = 546 + 96 * 2 + 8 * proofs.shape[1] + 96
    kept = 3 * (516 + g + 96 * 2 + TB[curve])
    try:
        whole = vk.test_fold_segment_parts(proofs, inputs, rho)
        assert gpu.api.test_fold_locate_last_chunks() == 1
        assert list(whole["verdicts"]) == [2 if j == g else 0 for j in range(n)] and list(whole["accepted"]) == [1, 0, 1]
        # (the recheck runs under the same cap: the smallest one here still holds tens of proofs of the per-proof verifier)
        for cap, chunks in ((kept + g * per_proof, 3), (kept + 2 * g * per_proof, 2), (kept + g * per_proof // 2, 3), (kept + 2 * g * per_proof - 1, 3)):
            vk.set_workspace_cap(cap)
            pieces = vk.test_fold_segment_parts(proofs, inputs, rho)
            assert gpu.api.test_fold_locate_last_chunks() == chunks, cap
            for part in ("f", "s", "t", "rho", "accepted", "status", "verdicts"):
                assert np.array_equal(pieces[part], whole[part]), (cap, part)
            assert pieces["report"]["segments_rejected"] == 1 and pieces["report"]["proofs_rechecked"] == g
    finally:
        vk.set_workspace_cap(0)
        vk.close()


@pytest.mark.parametrize("curve", [0, 1])
def test_device_pointers(gpu, curve):
    g = seg(gpu, curve)
    n = g + 1
    vk = TF.key(gpu, curve)
    proofs, inputs = TF.valid_batch(curve, n)
    bend(proofs, curve, n - 1)
    rho = TF.rhos(n)
    dp, di = gpu.DeviceBuffer.from_numpy(proofs), gpu.DeviceBuffer.from_numpy(inputs)
    verdicts, rep = vk.verify_folded_locate(dp.ptr.value, di.ptr.value, FR.coefficient_words(rho), on_device=True, n=n)
    host, host_rep = vk.verify_folded_locate(proofs, inputs, rho)
    assert list(verdicts) == list(host) == [0] * (n - 1) + [2]
    assert rep["segments_rejected"] == host_rep["segments_rejected"] == 1 and rep["proofs_rechecked"] == host_rep["proofs_rechecked"] == 1


@pytest.mark.parametrize("curve", [0, 1])
def test_device_pointers_with_two_separate_rejected_segments(gpu, curve):
    """n = 2 g + 1 on the device with C := A at 0 and at 2 g: segments 0 and 2 are rejected, 1 is not, so the recheck gathers two runs
    that are not adjacent from device memory into one batch and scatters its verdicts; then under a cap below that copy, where every
    run is verified where it lies"""
    g = seg(gpu, curve)
    n = 2 * g + 1
    alpha, beta, delta, abc, _, _ = TP.g16_key_parts(curve)
    vk = gpu.VerificationKey(curve, alpha, beta, delta, abc)
    proofs, inputs = TF.valid_batch(curve, n)
    bend(proofs, curve, 0)
    bend(proofs, curve, 2 * g)
    rho = TF.rhos(n)
    want = [2] + [0] * (2 * g - 1) + [2]
    dp, di = gpu.DeviceBuffer.from_numpy(proofs), gpu.DeviceBuffer.from_numpy(inputs)
    try:
        assert list(vk.verify(proofs, inputs, check_subgroup=True)) == want
        for cap in (0, (g + 1) * (8 * proofs.shape[1] + 96) - 1):           # (the second: one byte less than the gathered copy)
            vk.set_workspace_cap(cap)
            verdicts, rep = vk.verify_folded_locate(dp.ptr.value, di.ptr.value, FR.coefficient_words(rho), on_device=True, n=n)
            assert list(verdicts) == want, cap
            assert (rep["segments"], rep["segments_rejected"], rep["proofs_rechecked"]) == (3, 2, g + 1), (cap, rep)
    finally:
        vk.set_workspace_cap(0)
        vk.close()


@pytest.mark.parametrize("curve", [0, 1])
def test_errors_and_the_empty_batch(gpu, curve):
    vk = TF.key(gpu, curve)
    proofs, inputs = TF.valid_batch(curve, 3)
    with pytest.raises(gpu.Mnt753Error, match="coefficient is zero"):
        vk.verify_folded_locate(proofs, inputs, [5, 0, 7])
    L = gpu.api.lib()
    co = FR.coefficient_words([5, 6, 7])
    u64p = C.POINTER(C.c_uint64)
    verdicts = np.zeros(3, dtype=np.uint8)
    args = (vk._h, C.c_void_p(proofs.ctypes.data), C.c_void_p(inputs.ctypes.data))
    assert L.mnt753_groth16_verify_folded_locate(*args, 3, 0, co.ctypes.data_as(u64p), None, None, None) == EINVAL          # no verdicts
    assert L.mnt753_groth16_verify_folded_locate(*args, (1 << 24) + 1, 0, co.ctypes.data_as(u64p), C.c_void_p(verdicts.ctypes.data), None, None) == EINVAL
    assert L.mnt753_groth16_verify_folded_locate(*args, 3, 0, None, C.c_void_p(verdicts.ctypes.data), None, None) == EINVAL  # no coefficients
    assert L.mnt753_groth16_verify_folded_locate(*args, 0, 0, co.ctypes.data_as(u64p), C.c_void_p(verdicts.ctypes.data), None, None) == 0
    empty, rep = vk.verify_folded_locate(np.zeros((0, proofs.shape[1]), dtype=np.uint64), np.zeros((0, 12), dtype=np.uint64), [], n=0)
    assert empty.size == 0 and rep["segments"] == 0
    drawn, rep = vk.verify_folded_locate(proofs, inputs)                    # coefficients drawn by the wrapper
    assert not drawn.any() and rep["segments"] == 1


@pytest.mark.parametrize("curve", [0, 1])
def test_cli_fold_locate(gpu, curve, tmp_path):
    """main_hip verify --fold-locate: the good proof g times and a bad one once -> exit 3, g VERIFIED lines and REJECTED last, the
    summary on stderr; only good files -> exit 0; --fold and --compressed beside it are refused with exit 2"""
    g = seg(gpu, curve)
    el = TP.g16_elements_file(curve, tmp_path)
    inp, full = TP.g16(curve, "input.bin"), TP.g16(curve, "full.bin")
    proof = np.fromfile(full, dtype="<u8")
    proof[24 + W2[curve]:] = proof[:24]
    bent = tmp_path / "bent.bin"
    proof.astype("<u8").tofile(bent)
    cli = lambda args: subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True)
    r = cli([NAME[curve], "verify", el, inp] + [full] * g + [bent, "--fold-locate"])
    assert (r.returncode, r.stdout.splitlines()) == (3, ["VERIFIED"] * g + ["REJECTED"]), r.stdout + r.stderr
    assert "fold: 2 segments, 1 rejected, 1 proofs rechecked" in r.stderr.splitlines()
    r = cli([NAME[curve], "verify", el, inp, full, full, "--fold-locate"])
    assert (r.returncode, r.stdout.splitlines()) == (0, ["VERIFIED", "VERIFIED"]), r.stdout + r.stderr
    assert "fold: 1 segments, 0 rejected, 0 proofs rechecked" in r.stderr.splitlines()
    for other in ("--fold", "--compressed"):
        r = cli([NAME[curve], "verify", el, inp, full, other, "--fold-locate"])
        assert r.returncode == 2 and r.stdout == "" and "--fold-locate" in r.stderr, other
