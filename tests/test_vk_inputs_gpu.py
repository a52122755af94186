"""GPU: the input tables of a verification key (mnt753_vk_prepare_inputs).  A prepared key must give, word for
word, what an unprepared key gives -- the accumulated points, the verdicts of every verifier, the parts of the fold -- and what an
independent expectation says.  Everything is bit-exact; there is no tolerance.

Keys with many inputs come from the committed g16 fixtures (one input x, a proof the verifier accepts), widened as
tests/vk_inputs_ref.py describes: ABC'_j = a_j ABC_1 and inputs that combine to x, so the committed proofs stay valid and a wrong
base index shows.  The expectation of an accumulation is ABC_0 + (sum x_j a_j mod r) ABC_1 through point_scale / point_add /
point_to_affine on the host, none of which the tables touch.

Shapes: k in {1, 2, 3, 33, 257} inputs, n in {1, 2, 65, 257} proofs (a wave and one, a workgroup and one), widths {2, 3, default, 8},
and slices of 1, 2, k - 1 and k inputs per lane forced through the test library (a ragged last slice, a single slice)."""
import functools
import subprocess

import numpy as np
import pytest

import batch_exp_ref as BR
import pyref
import test_pairing_gpu as TP
import vk_inputs_ref as VR
from test_groth16_cpu import EXE, NAME

pytestmark = pytest.mark.gpu

W2 = {0: 48, 1: 72}


def pkg():
    from __graft_entry__ import load_package
    return load_package()


def fr(curve):
    return TP.model(curve).C


def words(curve, ints):
    C = fr(curve)
    return np.array([C.fr_to_words(int(v) % C.r) for v in ints], dtype=np.uint64).reshape(len(ints), 12)


def raw(v):
    return np.array([(v >> (64 * i)) & (2 ** 64 - 1) for i in range(12)], dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def widened(curve, k, a0=None):
    """-> (a_1 .. a_k, ABC' [k + 1, 24]); a0: ABC'_0 = a0 ABC_1 instead of the fixture's ABC_0"""
    gpu = pkg()
    C = fr(curve)
    abc = TP.g16_key_parts(curve)[3].reshape(2, 24)
    a = VR.ratios(C.r, k, 1000 * curve + k)
    fb = gpu.FixedBase(curve, 1, abc[1])
    pts = fb.batch_exp(words(curve, ([a0] if a0 is not None else []) + a))
    fb.close()
    first = abc[:1] if a0 is None else pts[:1]
    out = np.concatenate([first, pts[(0 if a0 is None else 1):]])
    out.setflags(write=False)
    return tuple(a), out


def make_key(gpu, curve, k, a0=None):
    alpha, beta, delta, _, _, _ = TP.g16_key_parts(curve)
    return gpu.VerificationKey(curve, alpha, beta, delta, widened(curve, k, a0)[1].reshape(-1))


def fixture_x(curve):
    C = fr(curve)
    return C.fr_from_words([int(v) for v in TP.g16_key_parts(curve)[5]])


@functools.lru_cache(maxsize=None)
def input_rows(curve, k, n):
    """n rows of k inputs that all combine to the fixture's x: the designed rows first, then random ones -> list of lists"""
    C = fr(curve)
    a = list(widened(curve, k)[0])
    x = fixture_x(curve)
    rows = [r for _, r in VR.designed_rows(C.r, a, x, BR.wrap_family(curve))]
    rng = pyref.splitmix64(77 + curve + 10 * k)
    while len(rows) < n:
        head = [pyref.rand_below(rng, C.r) for _ in range(k - 1)]
        rows.append(head + [VR.solve_last(C.r, a, head, x)])
    return rows[:n]


def rows_to_words(curve, rows):
    return np.stack([words(curve, r).reshape(-1) for r in rows])


def expected_points(gpu, curve, first_affine, base_affine, sums):
    """first + s base for every s, affine wire words, the identity as zero words: the host group law"""
    P0 = gpu.point_from_affine(curve, 1, first_affine)
    B = gpu.point_from_affine(curve, 1, base_affine)
    cache, out = {}, []
    for s in sums:
        if s not in cache:
            cache[s] = gpu.point_to_affine(curve, 1, gpu.point_add(curve, 1, P0, gpu.point_scale(curve, 1, words(curve, [s])[0], B)))
        out.append(cache[s])
    return np.stack(out)


_PLAIN = {}


def plain_accumulate(gpu, curve, k, n):
    """the accumulation of an UNPREPARED key object on input_rows(curve, k, n): today's kernel, once per shape"""
    if (curve, k, n) not in _PLAIN:
        vk = make_key(gpu, curve, k)
        assert not vk.input_plan()["prepared"]
        _PLAIN[(curve, k, n)] = vk.accumulate(rows_to_words(curve, input_rows(curve, k, n)).reshape(n, k, 12))
        vk.close()
    return _PLAIN[(curve, k, n)]


def check_accumulate(gpu, curve, k, n, w, ipl):
    C = fr(curve)
    a, abc = widened(curve, k)
    rows = input_rows(curve, k, n)
    vk = make_key(gpu, curve, k)
    plan = vk.prepare_inputs(window_bits=w)
    want_w = w or VR.default_window_bits(k + 1)
    assert plan == vk.input_plan() and plan["prepared"] and plan["window_bits"] == want_w and plan["windows"] == VR.windows(want_w)
    assert plan["table_bytes"] == VR.table_bytes(k + 1, want_w)
    assert vk.input_plan(n)["inputs_per_lane"] == VR.inputs_per_lane(n, k)
    if ipl:
        vk.test_force_inputs_per_lane(ipl)
        assert vk.input_plan(n)["inputs_per_lane"] == min(ipl, k)
    got = vk.accumulate(rows_to_words(curve, rows).reshape(n, k, 12))
    vk.close()
    base = TP.g16_key_parts(curve)[3].reshape(2, 24)
    want = expected_points(gpu, curve, abc[0], base[1], [VR.combined(C.r, a, r) for r in rows])
    assert np.array_equal(got, want), np.nonzero((got != want).any(axis=1))[0][:8]
    assert np.array_equal(got, plain_accumulate(gpu, curve, k, n))


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("k", [1, 2, 3, 33, 257])
def test_accumulate_every_number_of_inputs(gpu, curve, k):
    """n = 65 (a wave and one) at the default width and the host's slices; k = 257: n = 2, two slices of the walk's choice"""
    check_accumulate(gpu, curve, k, 65 if k < 257 else 2, 0, 0)


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 257])
def test_accumulate_every_number_of_proofs(gpu, curve, n):
    check_accumulate(gpu, curve, 3, n, 0, 0)
    check_accumulate(gpu, curve, 33, n, 0, 2)


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("w", [2, 3, 8])
def test_accumulate_every_width(gpu, curve, w):
    check_accumulate(gpu, curve, 33, 2, w, 0)
    check_accumulate(gpu, curve, 3, 65, w, 1)


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("k", [3, 33, 257])
def test_accumulate_every_slice_size(gpu, curve, k):
    """1, 2, k - 1 and k inputs per lane: k, ceil(k / 2), two (the last of one input) and one partial sum per proof.  At one input
    per lane the designed rows put equal and opposite partial sums side by side: the segment sum must double and must cancel.
    (k = 257 at n = 2 and the default width 6: a lane that walks 256 or 257 inputs does 32000 additions in a row, about 1.5 s.)"""
    n = 65 if k < 257 else 2
    for ipl in (1, 2, k - 1, k):
        check_accumulate(gpu, curve, k, n, 0, ipl)


@pytest.mark.parametrize("curve", [0, 1])
def test_all_zero_row_and_identity_sum(gpu, curve):
    """an all-zero row accumulates to ABC_0; with ABC'_0 = a_0 ABC_1 a row with sum x_j a_j = -a_0 accumulates to the identity: zero
    words from mnt753_vk_accumulate, verdict 1 from the verifier, prepared or not"""
    C = fr(curve)
    k, a0 = 3, 0xABCDEF
    a, abc = widened(curve, k, a0)
    head = [5, C.r - 9]
    to_identity = head + [VR.solve_last(C.r, list(a), head, C.r - a0)]
    rows = [[0, 0, 0], to_identity, [1, 2, 3], [0, 0, 0]]
    inputs = rows_to_words(curve, rows)
    base = TP.g16_key_parts(curve)[3].reshape(2, 24)
    want = expected_points(gpu, curve, np.zeros(24, dtype=np.uint64), base[1], [(a0 + VR.combined(C.r, a, r)) % C.r for r in rows])
    assert not want[1].any() and np.array_equal(want[0], abc[0])
    proofs = np.tile(TP.g16_key_parts(curve)[4], (4, 1))
    plain, prepared = make_key(gpu, curve, k, a0), make_key(gpu, curve, k, a0)
    prepared.prepare_inputs()
    for ipl in (0, 1, 2, 3):
        prepared.test_force_inputs_per_lane(ipl)
        got = prepared.accumulate(inputs.reshape(4, k, 12))
        assert np.array_equal(got, want) and np.array_equal(got, plain.accumulate(inputs.reshape(4, k, 12))), ipl
        v = prepared.verify(proofs, inputs)
        assert v[1] == 1 and list(v) == list(plain.verify(proofs, inputs)), ipl
    plain.close(); prepared.close()


def widened_batch(curve, k, n):
    """TP.build_batch -- planted invalid proofs at the edges, malformed ones in slots 1 .. 9, an input >= r in slot 4 -- with every
    row's single input x_i widened to k inputs that combine to it; the row with the input >= r keeps it in the middle"""
    C = fr(curve)
    a = list(widened(curve, k)[0])
    proofs, inputs, want = TP.build_batch(curve, n)
    rng = pyref.splitmix64(5 + curve + k)
    rows = []
    for i in range(n):
        xi = sum(int(v) << (64 * j) for j, v in enumerate(inputs[i]))          # the stored (Montgomery) integer
        head = [pyref.rand_below(rng, C.r) for _ in range(k - 1)]
        if xi >= C.r:
            row = rows_to_words(curve, [head + [1]])[0]
            row[12 * (k // 2):12 * (k // 2) + 12] = raw(C.r)
        else:
            x = C.fr_from_words([int(v) for v in inputs[i]])
            row = rows_to_words(curve, [head + [VR.solve_last(C.r, a, head, x)]])[0]
        rows.append(row)
    return proofs, np.stack(rows), want


def compress_proofs(gpu, curve, proofs):
    w2 = W2[curve]
    xa, fa = gpu.compress_points(curve, 1, proofs[:, :24].copy())
    xb, fb = gpu.compress_points(curve, 2, proofs[:, 24:24 + w2].copy())
    xc, fc = gpu.compress_points(curve, 1, proofs[:, 24 + w2:].copy())
    n = proofs.shape[0]
    return np.concatenate([xa.reshape(n, -1), xb.reshape(n, -1), xc.reshape(n, -1)], axis=1), np.stack([fa, fb, fc], axis=1).astype(np.uint8)


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("k", [3, 33])
def test_verdicts_of_every_verifier(gpu, curve, k):
    """verify, verify(check_subgroup), verify_compressed and verify_folded on a batch with accepted, invalid and malformed proofs at
    the edges and an input >= r in the middle: the prepared key's bytes are the unprepared key's, and verify's are build_batch's"""
    n = 65
    proofs, inputs, want = widened_batch(curve, k, n)
    plain, prepared = make_key(gpu, curve, k), make_key(gpu, curve, k)
    prepared.prepare_inputs()
    x, flags = compress_proofs(gpu, curve, proofs)
    rho = [3 + 2 * i + (1 << 127) for i in range(n)]
    good = np.nonzero(want == 0)[0]
    p_plain, p_sub, p_comp = plain.verify(proofs, inputs), plain.verify(proofs, inputs, check_subgroup=True), plain.verify_compressed(x, flags, inputs)
    p_fold, p_fold_good = plain.verify_folded(proofs, inputs, rho), plain.verify_folded(proofs[good], inputs[good], rho[:len(good)])
    assert list(p_plain) == list(want) and p_fold[0] is False and p_fold_good[0] is True and not p_fold_good[1].any()
    for ipl in ((0, 2) if k == 3 else (2,)):                                 # (k = 33, n = 65: the host's choice is one input per lane)
        prepared.test_force_inputs_per_lane(ipl)
        assert list(prepared.verify(proofs, inputs)) == list(want)
        assert list(prepared.verify(proofs, inputs, check_subgroup=True)) == list(p_sub)
        assert list(prepared.verify_compressed(x, flags, inputs)) == list(p_comp)
        accepted, status = prepared.verify_folded(proofs, inputs, rho)
        assert accepted is False and list(status) == list(p_fold[1])
        accepted, status = prepared.verify_folded(proofs[good], inputs[good], rho[:len(good)])
        assert accepted is True and not status.any()
    plain.close(); prepared.close()


@pytest.mark.parametrize("curve", [0, 1])
def test_verdicts_in_chunks_under_a_workspace_cap(gpu, curve):
    """a cap that leaves about five proofs per chunk, and one below a single proof (chunks of one): the inputs per lane are then
    chosen again for the chunk that runs -- more slices per proof, which shrink the chunk once more -- and the verdicts are
    build_batch's"""
    k, n = 33, 22
    proofs, inputs, want = widened_batch(curve, k, n)
    vk = make_key(gpu, curve, k)
    vk.prepare_inputs()
    vk.set_workspace_cap(5 * (194 + 96 * k + 8 * proofs.shape[1] + 96 * k + VR.workspace_per_proof(k, 1)))
    assert list(vk.verify(proofs, inputs)) == list(want)
    assert list(vk.verify(proofs, inputs, check_subgroup=True)) == list(want)
    vk.set_workspace_cap(1)
    assert list(vk.verify(proofs[:3], inputs[:3])) == list(want[:3])
    vk.set_workspace_cap(0)
    assert list(vk.verify(proofs, inputs)) == list(want)
    vk.close()


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("k", [3, 33])
@pytest.mark.parametrize("n", [1, 3])
def test_fold_parts(gpu, curve, k, n):
    """S, T, rho and F of the test_fold_parts hook are equal between the two keys, for the host's slices of the walk that forms S and
    for forced ones, and in chunks of one proof (the column sums carried from chunk to chunk)"""
    rows = input_rows(curve, k, n)
    inputs = rows_to_words(curve, rows)
    proofs = TP.proof_pool(curve)[0][np.arange(n) % TP.NP].copy()
    rho = [(1 << 127) | 12345, 1, (1 << 128) - 1][:n]
    plain, prepared = make_key(gpu, curve, k), make_key(gpu, curve, k)
    prepared.prepare_inputs()
    want = plain.test_fold_parts(proofs, inputs, rho)
    assert want["accepted"]
    for ipl, cap in ((0, 0), (1, 0), (k, 0), (2, 1)):
        prepared.test_force_inputs_per_lane(ipl)
        prepared.set_workspace_cap(cap)
        got = prepared.test_fold_parts(proofs, inputs, rho)
        assert got["accepted"] and all(np.array_equal(got[f], want[f]) for f in ("s", "t", "rho", "f", "status")), (ipl, cap)
    plain.close(); prepared.close()


@pytest.mark.parametrize("curve", [0, 1])
def test_refusals_release_and_replacement(gpu, curve):
    """a width whose tables exceed a small cap, widths 1 and 17 and a key without inputs are refused with a message that names the
    bytes and the cap, and leave a prepared key working; preparing again replaces the tables; release_inputs returns the key to
    today's path and the plan says so"""
    k, n = 3, 2
    vk = make_key(gpu, curve, k)
    inputs = rows_to_words(curve, input_rows(curve, k, n)).reshape(n, k, 12)
    want = plain_accumulate(gpu, curve, k, n)
    assert vk.input_plan() == {"prepared": False, "window_bits": 0, "windows": 0, "inputs_per_lane": 0, "table_bytes": 0}
    first = vk.prepare_inputs(window_bits=3)
    assert first["window_bits"] == 3 and first["table_bytes"] == VR.table_bytes(k + 1, 3)
    need, cap = VR.table_bytes(k + 1, 8), VR.table_bytes(k + 1, 8) - 1
    with pytest.raises(gpu.Mnt753Error, match=f"{need} bytes.*{cap} bytes"):
        vk.prepare_inputs(window_bits=8, max_table_bytes=cap)
    with pytest.raises(gpu.Mnt753Error, match=f"{VR.table_bytes(k + 1, 2)} bytes.*cap is 1000 bytes"):
        vk.prepare_inputs(max_table_bytes=1000)
    for w in (1, 17, -2):
        with pytest.raises(gpu.Mnt753Error, match="window_bits"):
            vk.prepare_inputs(window_bits=w)
    assert vk.input_plan() == first and np.array_equal(vk.accumulate(inputs), want)
    small = vk.prepare_inputs(max_table_bytes=VR.table_bytes(k + 1, 5))      # the widest width under a cap: replaces the tables
    assert small["window_bits"] == 5 and np.array_equal(vk.accumulate(inputs), want)
    vk.release_inputs()
    assert not vk.input_plan()["prepared"] and np.array_equal(vk.accumulate(inputs), want)
    vk.release_inputs()                                                      # twice is fine
    vk.close()
    alpha, beta, delta, abc, _, _ = TP.g16_key_parts(curve)
    none = gpu.VerificationKey(curve, alpha, beta, delta, abc[:24])
    with pytest.raises(gpu.Mnt753Error, match="no public inputs"):
        none.prepare_inputs()
    assert not none.input_plan()["prepared"]
    none.close()


@pytest.mark.parametrize("curve", [0, 1])
def test_input_not_below_r_is_an_error_of_accumulate(gpu, curve):
    k = 3
    vk = make_key(gpu, curve, k)
    vk.prepare_inputs()
    inputs = rows_to_words(curve, input_rows(curve, k, 3)).reshape(3, k, 12).copy()
    inputs[1, 1] = raw(fr(curve).r)
    with pytest.raises(gpu.Mnt753Error, match="not below r"):
        vk.accumulate(inputs)
    vk.close()


@pytest.mark.parametrize("curve", [0, 1])
def test_cli_input_tables(gpu, curve, tmp_path):
    """main_hip verify on a key with three inputs: the same lines and exit codes with and without --input-tables, also under --fold,
    --check-subgroup and --compressed; the plan line unless --quiet; exit 2 for a width that is none"""
    k = 3
    alpha, beta, delta, _, proof, _ = TP.g16_key_parts(curve)
    el = tmp_path / "vk_elements.bin"
    np.concatenate([alpha, beta, delta, widened(curve, k)[1].reshape(-1)]).astype("<u8").tofile(el)
    inp = tmp_path / "input.bin"
    one = words(curve, [1])
    np.concatenate([one.reshape(-1), rows_to_words(curve, input_rows(curve, k, 1))[0]]).astype("<u8").tofile(inp)
    full = TP.g16(curve, "full.bin")
    bent = tmp_path / "bent.bin"
    b = proof.copy()
    b[24 + W2[curve]:] = b[:24]
    b.astype("<u8").tofile(bent)
    cli = lambda args: subprocess.run([EXE, NAME[curve], "verify", str(el), str(inp)] + [str(a) for a in args], capture_output=True, text=True)
    two = ["VERIFIED", "REJECTED"]
    for extra, files, code, lines, compare in (([], [full, bent], 3, two, True), (["--fold"], [full, bent], 3, two, True),
                                               (["--fold"], [full], 0, ["VERIFIED 1 proofs (folded)"], False), (["--check-subgroup"], [full], 0, ["VERIFIED"], False)):
        got = cli(files + extra + ["--input-tables", "--quiet"])
        assert (got.returncode, got.stdout.splitlines()) == (code, lines), (extra, got.stdout + got.stderr)
        if compare:
            want = cli(files + extra)
            assert (got.returncode, got.stdout) == (want.returncode, want.stdout), (extra, want.stdout + want.stderr)
    got = cli([full, "--input-tables", "--input-window-bits", "4"])
    assert got.returncode == 0 and got.stdout.splitlines() == [f"input tables: w = 4, W = 189, {VR.table_bytes(k + 1, 4)} bytes", "VERIFIED"], got.stdout + got.stderr
    for bad in ("1", "17", "x"):
        r = cli([full, "--input-tables", "--input-window-bits", bad])
        assert r.returncode == 2 and "--input-window-bits" in r.stderr
    comp = tmp_path / "full.z"
    r = subprocess.run([EXE, NAME[curve], "compress-proof", full, str(comp)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = cli([comp, "--compressed", "--input-tables", "--quiet"])
    assert (got.returncode, got.stdout) == (0, "VERIFIED\n"), got.stdout + got.stderr
