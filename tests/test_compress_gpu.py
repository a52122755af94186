"""GPU: compressed points on the device (include/mnt753_hip.h "compressed points") against the Python-integer
reference of tests/compress_ref.py, which tests/test_compress_cpu.py checks against streams written by libff with point compression
on (tests/golden/compress/).  Every comparison is exact.

Shapes: one lane per G1 point -- 64 per wave, 256 per workgroup --, one lane group per G2 point -- g = 32 per wave and 128 per workgroup
on MNT4753, 21 and 84 on MNT6753 (lane 63 idles) --, so the sizes are 0, 1, 2, one wave's worth, one more, and four waves' worth plus
one, and a bad element sits at index 0, in the last slot of a wave, in the first slot of the next one and at n - 1.  The square-root
hook runs a DESIGNED set (compress_ref.sqrt_designed_set): random squares almost never reach the shallow Tonelli-Shanks depths."""
import functools
import os
import subprocess

import numpy as np
import pytest

import compress_ref as CR
import designed_points as DP
import keygen_ref as K
import subgroup_ref as S
import test_pairing_gpu as TP
import test_subgroup_gpu as TS
import validate_ref as V
from test_compress_cpu import FIX, IDENTITY_AT, fixture, proof_fixture
from test_groth16_cpu import EXE, NAME

pytestmark = pytest.mark.gpu

PER_WAVE = {(c, g): (64 if g == 1 else S.GROUPS_PER_WAVE[c]) for c, g in CR.GROUPS}
SIZES = {k: [0, 1, 2, w, w + 1, 4 * w + 1] for k, w in PER_WAVE.items()}
CASES = [(c, g, n) for (c, g) in CR.GROUPS for n in SIZES[(c, g)]]


def raw(v):
    return np.array([(v >> (64 * i)) & (2 ** 64 - 1) for i in range(12)], dtype=np.uint64)


def edges(curve, group, n):
    w = PER_WAVE[(curve, group)]
    return sorted({0, w - 1, w, n - 1} & set(range(n)))


# ---- the square root on raw field elements ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sqrt_set(curve, deg):
    return CR.sqrt_designed_set(curve, deg)


@pytest.mark.parametrize("curve,deg", [(0, 1), (1, 1), (0, 2), (1, 3)])
@pytest.mark.parametrize("window", [None, 1, 2, 4])
def test_square_root_on_the_designed_set(gpu, curve, deg, window):
    """is_square exact and r^2 = a exact for every Tonelli-Shanks depth k = 0 .. s - 1, for 0, 1, q - 1, the all-(q - 1) element and
    for the non-squares, neighbours in a wave at different depths; the set repeated across a wave and a workgroup boundary.  window:
    the product's own (None) and each alternative of the fixed exponent's window."""
    cv = CR.CURVES[curve]
    base = sqrt_set(curve, deg)
    s = CR.two_adic(curve, deg)[0]
    assert [name for name, _, _ in base if name.startswith("depth")] and sum(name.startswith("depth") for name, _, _ in base) == s
    group = 1 if deg == 1 else 2
    n = 4 * PER_WAVE[(curve, group)] + 1
    picks = [base[i % len(base)] for i in range(n)]
    words = np.array([cv.coord_to_words(a) for _, a, _ in picks], dtype=np.uint64)
    got = gpu.api.test_field_sqrt(curve, deg, words, window=window)
    roots, is_square = got[0], got[1]
    assert list(is_square) == [int(sq) for _, _, sq in picks]
    for i, (name, a, sq) in enumerate(picks):
        if not sq:
            assert not roots[i].any(), (i, name)
            continue
        r = cv.coord_from_words([int(v) for v in roots[i]], deg)
        assert cv.f_mul(r, r) == a, (i, name)
    # the same elements give the same roots wherever they sit
    for i in range(len(base), n):
        assert np.array_equal(roots[i], roots[i - len(base)]), i


# ---- decompress: sizes and positions ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def good_pool(curve, group):
    """distinct good points as pyref points (None: the identity): generator multiples, the designed families, the identity"""
    cv = CR.CURVES[curve]
    G = cv.gen(group)
    pts = [G, cv.neg(G)] + [cv.mul(k, G, group) for k in (2, 3, 0xABCDEF, cv.r - 2)]
    if group == 1:
        pts += list(DP.edge_points(curve).values())
    else:
        pts += [pt for _, pt in DP.sparse_points(curve)]
    for tri in DP.same_y_triples(curve, group):
        pts += list(tri) + [cv.neg(tri[0])]
    pts.insert(3, None)
    assert all(p is None or cv.on_curve(p, group) for p in pts)
    return tuple(pts)


@functools.lru_cache(maxsize=None)
def good_words(curve, group):
    """-> points [m, 2 Wx], x [m, Wx], flags [m] of the pool (the reference's compression)"""
    pts = np.stack([DP.to_words(curve, group, p) for p in good_pool(curve, group)])
    x, flags = CR.compress(curve, group, pts)
    return pts, x, flags


def good_batch(curve, group, n):
    pts, x, flags = good_words(curve, group)
    idx = np.arange(n) % len(pts)
    return pts[idx].copy(), x[idx].copy(), flags[idx].copy()


def bad_kinds(curve, group):
    """[(x words, flag or None = keep, reason)]: a non-liftable x, x = q, x = 2^768 - 1, flag 4"""
    wx = CR.x_words(curve, group)
    q = CR.CURVES[curve].q
    xq = np.zeros(wx, dtype=np.uint64); xq[wx - 12:] = raw(q)                      # the LAST component = q: another lane's word
    ones = np.full(wx, 2 ** 64 - 1, dtype=np.uint64)
    return [(CR.non_liftable_words(curve, group), None, CR.BAD_OFF_CURVE), (xq, None, CR.BAD_NONCANONICAL), (ones, None, CR.BAD_NONCANONICAL),
            (None, 4, CR.BAD_NONCANONICAL)]


def plant(x, flags, i, kind):
    bx, bf, _ = kind
    if bx is not None:
        x[i] = bx
        flags[i] &= 1                                                             # a point's flag, so that the x decides
    if bf is not None:
        flags[i] = bf


@pytest.mark.parametrize("curve,group,n", CASES)
def test_decompress_sizes_and_positions(gpu, curve, group, n):
    wx = CR.x_words(curve, group)
    pts, x, flags = good_batch(curve, group, n)
    assert set(int(f) for f in good_words(curve, group)[2]) == {0, 1, 2}
    got, rep = gpu.decompress_points(curve, group, x.reshape(-1) if n else np.zeros(0, dtype=np.uint64), flags, n=n)
    assert rep == (0, 0, 0) and got.shape == (n, 2 * wx) and np.array_equal(got, pts)
    if n == 0:
        return
    kinds = bad_kinds(curve, group)
    for i in edges(curve, group, n):
        for kind in kinds:
            bx, bf = x.copy(), flags.copy()
            plant(bx, bf, i, kind)
            got, rep = gpu.decompress_points(curve, group, bx, bf)
            assert rep == (1, i, kind[2]), (n, i, kind[2])
            want = pts.copy(); want[i] = 0
            assert np.array_equal(got, want), (n, i)                               # the planted slot zero, every neighbour intact
    for kind in kinds:                                                            # all bad
        bx, bf = x.copy(), flags.copy()
        for i in range(n):
            plant(bx, bf, i, kind)
        got, rep = gpu.decompress_points(curve, group, bx, bf)
        assert rep == (n, 0, kind[2]) and not got.any()
    # several at once, a different kind in each edge slot: the lowest index and its reason
    bx, bf = x.copy(), flags.copy()
    es = edges(curve, group, n)
    for k, i in enumerate(es):
        plant(bx, bf, i, kinds[(k + 1) % len(kinds)])
    got, rep = gpu.decompress_points(curve, group, bx, bf)
    assert rep == (len(es), es[0], kinds[1 % len(kinds)][2])
    want = pts.copy(); want[es] = 0
    assert np.array_equal(got, want)


@pytest.mark.parametrize("curve,group", CR.GROUPS)
def test_decompress_precedence_per_point(gpu, curve, group):
    """non-canonical before the identity before off-curve, per point; the other parity gives the other root"""
    cv = CR.CURVES[curve]
    wx = CR.x_words(curve, group)
    good_x, good_f = CR.compress_point(curve, group, cv.gen(group))
    bad_x = [int(v) for v in CR.non_liftable_words(curve, group)]
    q_words = [int(v) for v in raw(cv.q)] + [0] * (wx - 12)
    rows = [(good_x, good_f), (bad_x, 0), (bad_x, 1), (bad_x, 2), (bad_x, 4), (q_words, 0), (q_words, 2), (q_words, 6), (good_x, 6), (good_x, 2),
            (good_x, 0x80 | good_f), (good_x, good_f ^ 1), (bad_x, 3), (q_words, 3)]
    x = np.array([r[0] for r in rows], dtype=np.uint64)
    f = np.array([r[1] for r in rows], dtype=np.uint8)
    want, want_rep = CR.decompress(curve, group, x, f)
    got, rep = gpu.decompress_points(curve, group, x, f)
    assert rep == want_rep and np.array_equal(got, want)
    assert np.array_equal(got[11], DP.to_words(curve, group, cv.neg(cv.gen(group))))
    for i in range(len(rows)):                                                    # each alone: its own reason
        _, rep = gpu.decompress_points(curve, group, x[i], f[i:i + 1])
        assert rep == CR.decompress(curve, group, x[i], f[i:i + 1])[1], i


@pytest.mark.parametrize("curve,group", CR.GROUPS)
def test_compress_vs_reference(gpu, curve, group):
    """compress validates nothing: good points, the identity, and a point off its curve as it stands"""
    pts, x, flags = good_batch(curve, group, 4 * PER_WAVE[(curve, group)] + 1)
    off = pts[1].copy(); off[CR.x_words(curve, group)] ^= np.uint64(2)           # y changed: off the curve, compressed all the same
    pts[7] = off
    wx, wf = CR.compress(curve, group, pts)
    gx, gf = gpu.compress_points(curve, group, pts)
    assert np.array_equal(gx, wx) and np.array_equal(gf, wf)
    gx, gf = gpu.compress_points(curve, group, np.zeros(0, dtype=np.uint64), n=0)
    assert gx.shape == (0, CR.x_words(curve, group)) and gf.shape == (0,)


# ---- the sets of the committed parameter files, on device pointers ----------------------------------------------------------------------
def committed_sets(curve, group):
    """[(name, points [n, words])]: the sets of tests/golden/g16_mnt*/params.bin and of keygen_*/vk_elements.bin of this group"""
    out = []
    _, _, sets = V.params_sets(curve, TP.g16(curve, "params.bin"))
    for name, (g, _, n, pts) in sets.items():
        if g == group:
            out.append((f"g16/{name}", np.ascontiguousarray(pts, dtype=np.uint64).reshape(n, -1)))
    w2 = 24 * CR.CURVES[curve].deg
    for tag in ("full", "cut21"):
        el = TP.elements(curve, tag)
        if group == 1:
            out.append((f"keygen_{tag}/alpha|ABC", np.concatenate([el[:24], el[24 + 2 * w2:]]).reshape(-1, 24)))
        else:
            out.append((f"keygen_{tag}/beta|delta", el[24:24 + 2 * w2].reshape(2, w2)))
    return out


@pytest.mark.parametrize("curve,group", CR.GROUPS)
def test_round_trip_on_device_pointers(gpu, curve, group):
    wx = CR.x_words(curve, group)
    for name, pts in committed_sets(curve, group):
        n = len(pts)
        d_in = gpu.DeviceBuffer.from_numpy(pts)
        d_x, d_f, d_out = gpu.DeviceBuffer(8 * wx * n), gpu.DeviceBuffer((n + 15) // 16 * 16), gpu.DeviceBuffer(16 * wx * n)
        gpu.compress_points(curve, group, d_in.ptr.value, on_device=True, n=n, x_out=d_x.ptr.value, flags_out=d_f.ptr.value)
        x, flags = d_x.to_numpy().reshape(n, wx), d_f.to_numpy(np.uint8)[:n]
        rx, rf = CR.compress(curve, group, pts)
        assert np.array_equal(x, rx) and np.array_equal(flags, rf), name
        _, rep = gpu.decompress_points(curve, group, d_x.ptr.value, d_f.ptr.value, on_device=True, n=n, out=d_out.ptr.value)
        assert rep == (0, 0, 0), name
        assert np.array_equal(d_out.to_numpy().reshape(n, 2 * wx), pts), name
        bs = gpu.BaseSet(curve, group, d_out.ptr.value, on_device=True, n=n)      # straight into mnt753_bases_create
        assert bs.n == n
        bs.close()


@pytest.mark.parametrize("curve,group", CR.GROUPS)
def test_libff_fixture_on_the_device(gpu, curve, group):
    pts, stream = fixture(curve, group)
    x, flags = gpu.points_from_stream(curve, group, stream)
    got, rep = gpu.decompress_points(curve, group, x, flags)
    assert rep == (0, 0, 0) and np.array_equal(got, pts) and not got[IDENTITY_AT].any()
    cx, cf = gpu.compress_points(curve, group, pts)
    assert gpu.points_to_stream(curve, group, cx, cf) == stream


# ---- verify_compressed ------------------------------------------------------------------------------------------------------------------
def g16_key(gpu, curve):
    alpha, beta, delta, abc, _, _ = TP.g16_key_parts(curve)
    return gpu.VerificationKey(curve, alpha, beta, delta, abc)


@pytest.mark.parametrize("curve", [0, 1])
def test_verify_compressed_on_the_fixture_proofs(gpu, curve):
    w2 = 24 * CR.CURVES[curve].deg
    xw = 24 + w2 // 2
    vk = g16_key(gpu, curve)
    inp = TP.g16_key_parts(curve)[5]
    good, half = TP.proof_pool(curve)
    proofs = np.concatenate([good[:3], half[:1]])
    inputs = np.tile(inp, (len(proofs), 1))
    plain = vk.verify(proofs, inputs)
    assert list(plain) == [0, 0, 0, 2]
    x, flags = CR.compress_proofs(curve, proofs)
    assert x.shape == (4, xw) and flags.shape == (4, 3)
    gx, gf = gpu.compress_points(curve, 2, proofs[:, 24:24 + w2])                 # the device's compression of B agrees
    assert np.array_equal(gx, x[:, 12:12 + w2 // 2]) and np.array_equal(gf, flags[:, 1])
    assert list(vk.verify_compressed(x, flags, inputs)) == list(plain)
    assert list(vk.verify_compressed(x, flags, inputs, check_subgroup=True)) == list(plain)
    # the libff stream of the fixture's proof
    sx, sf = CR.proof_from_stream(curve, proof_fixture(curve)[1])
    assert list(vk.verify_compressed(sx, sf, inp)) == [0]
    # A's parity flipped: -A is a point, the pairing check fails
    f2 = flags.copy(); f2[0, 0] ^= 1
    assert list(vk.verify_compressed(x, f2, inputs)) == [2, 0, 0, 2]
    neg = proofs.copy()
    neg[0, :24] = DP.to_words(curve, 1, CR.CURVES[curve].neg(DP.from_words(curve, 1, proofs[0, :24])))
    assert list(vk.verify(neg, inputs)) == [2, 0, 0, 2]
    # a non-liftable x_B, an identity flag on C, a stray flag bit on A, x_C = q
    x3, f3 = x.copy(), flags.copy()
    x3[0, 12:12 + w2 // 2] = CR.non_liftable_words(curve, 2)
    f3[1, 2] = 2
    f3[2, 0] |= 8
    x3[3, 12 + w2 // 2:] = raw(CR.CURVES[curve].q)
    assert list(vk.verify_compressed(x3, f3, inputs)) == [1, 1, 1, 1]
    # from device memory
    dx, df, di = gpu.DeviceBuffer.from_numpy(x), gpu.DeviceBuffer.from_numpy(np.concatenate([flags.reshape(-1), np.zeros(4, dtype=np.uint8)])), \
        gpu.DeviceBuffer.from_numpy(inputs)
    assert list(vk.verify_compressed(dx.ptr.value, df.ptr.value, di.ptr.value, on_device=True, n=4)) == list(plain)
    vk.close()


@pytest.mark.parametrize("curve", [0, 1])
def test_verify_compressed_off_the_subgroup(gpu, curve):
    """B compressed from a twist point outside G2: 3 with check_subgroup, and without it whatever verify gives for the same point"""
    w2 = 24 * CR.CURVES[curve].deg
    vk = g16_key(gpu, curve)
    inp = TP.g16_key_parts(curve)[5]
    good, _ = TP.proof_pool(curve)
    proofs = good[:3].copy()
    proofs[1, 24:24 + w2] = TS.bad_b(curve)[0]
    proofs[2, 24:24 + w2] = TS.bad_b(curve)[1]
    inputs = np.tile(inp, (3, 1))
    x, flags = CR.compress_proofs(curve, proofs)
    assert list(vk.verify_compressed(x, flags, inputs, check_subgroup=True)) == [0, 3, 3]
    assert list(vk.verify_compressed(x, flags, inputs)) == list(vk.verify(proofs, inputs))
    vk.close()


@pytest.mark.parametrize("curve", [0, 1])
def test_verify_compressed_batch_with_tampered_wave_edges(gpu, curve):
    """g + 1 proofs, one tampered proof at each wave edge: the neighbours keep verdict 0; the same under a workspace cap"""
    w2 = 24 * CR.CURVES[curve].deg
    g = S.GROUPS_PER_WAVE[curve]
    n = g + 1
    vk = g16_key(gpu, curve)
    inp = TP.g16_key_parts(curve)[5]
    good, _ = TP.proof_pool(curve)
    proofs, inputs = good[np.arange(n) % TP.NP].copy(), np.tile(inp, (n, 1))
    x, flags = CR.compress_proofs(curve, proofs)
    want = np.zeros(n, dtype=np.uint8)
    flags[0, 0] ^= 1; want[0] = 2                                                 # -A
    x[g - 1, 12:12 + w2 // 2] = CR.non_liftable_words(curve, 2); want[g - 1] = 1  # the last slot of the wave
    flags[g, 2] = 2; want[g] = 1                                                  # the first slot of the next one: the identity as C
    assert list(vk.verify_compressed(x, flags, inputs)) == list(want)
    back = []
    for group, at, words in CR.proof_parts(curve):                                # decompress, then verify_ex: the same verdicts
        wx = CR.x_words(curve, group)
        xa = sum(CR.x_words(curve, gg) for gg, a2, _ in CR.proof_parts(curve) if a2 < at)
        k = [a2 for _, a2, _ in CR.proof_parts(curve)].index(at)
        back.append(gpu.decompress_points(curve, group, np.ascontiguousarray(x[:, xa:xa + wx]), np.ascontiguousarray(flags[:, k]))[0])
    assert list(vk.verify(np.concatenate(back, axis=1), inputs)) == list(want)
    vk.set_workspace_cap(5 * (194 + 96 + 8 * proofs.shape[1] + 8 * x.shape[1] + 3 + 96))
    assert list(vk.verify_compressed(x, flags, inputs)) == list(want)
    vk.set_workspace_cap(1)
    assert list(vk.verify_compressed(x[:3], flags[:3], inputs[:3])) == list(want[:3])
    vk.set_workspace_cap(0)
    vk.close()


# ---- the command line -------------------------------------------------------------------------------------------------------------------
def cli(args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True)


@pytest.mark.parametrize("curve", [0, 1])
def test_cli_on_the_fixture_proof(gpu, curve, tmp_path):
    w2 = 24 * CR.CURVES[curve].deg
    full, stream = TP.g16(curve, "full.bin"), proof_fixture(curve)[1]
    el, inp = TP.g16_elements_file(curve, tmp_path), TP.g16(curve, "input.bin")
    packed, back = tmp_path / "proof.z", tmp_path / "back.bin"
    r = cli([NAME[curve], "compress-proof", full, packed])
    assert r.returncode == 0 and packed.read_bytes() == stream, r.stderr
    r = cli([NAME[curve], "decompress-proof", packed, back])
    assert r.returncode == 0 and back.read_bytes() == open(full, "rb").read(), r.stderr
    r = cli([NAME[curve], "verify", el, inp, packed, packed, "--compressed"])
    assert (r.returncode, r.stdout.split()) == (0, ["VERIFIED", "VERIFIED"]), r.stdout + r.stderr
    flipped = bytearray(stream); flipped[97] ^= 1                                 # the parity byte of A: '0' <-> '1'
    (tmp_path / "flipped.z").write_bytes(bytes(flipped))
    r = cli([NAME[curve], "verify", el, inp, packed, tmp_path / "flipped.z", "--compressed", "--check-subgroup"])
    assert r.returncode == 3 and r.stdout.splitlines() == ["VERIFIED", "REJECTED"], r.stdout + r.stderr
    bad = bytearray(stream)
    bad[99:99 + 4 * w2] = CR.non_liftable_words(curve, 2).astype("<u8").tobytes()  # x of B
    (tmp_path / "bad.z").write_bytes(bytes(bad))
    r = cli([NAME[curve], "verify", el, inp, tmp_path / "bad.z", packed, "--compressed"])
    assert r.returncode == 3 and r.stdout.splitlines() == ["REJECTED (malformed)", "VERIFIED"], r.stdout + r.stderr
    out = tmp_path / "none.bin"
    r = cli([NAME[curve], "decompress-proof", tmp_path / "bad.z", out])
    assert r.returncode == 3 and "B: off curve" in r.stderr and not out.exists(), r.stderr
    noncanon = bytearray(stream)
    noncanon[1:97] = raw(CR.CURVES[curve].q).astype("<u8").tobytes()              # x of A = q
    (tmp_path / "nc.z").write_bytes(bytes(noncanon))
    r = cli([NAME[curve], "decompress-proof", tmp_path / "nc.z", out])
    assert r.returncode == 3 and "A: not canonical" in r.stderr and not out.exists(), r.stderr


@pytest.mark.parametrize("curve", [0, 1])
def test_cli_and_verify_compressed_on_a_generated_key(gpu, curve, tmp_path):
    """main_hip generate -> compute-r1cs -> complete (the keygen fixture's system) -> compress-proof -> verify --compressed, and the
    same proof through VerificationKey.verify_compressed next to verify"""
    outs, full, f = TP.cli_proof(curve, tmp_path, names=("good",))
    out = outs["good"]
    packed = tmp_path / "proof.z"
    assert cli([NAME[curve], "compress-proof", full, packed]).returncode == 0
    r = cli([NAME[curve], "verify", out / "vk_elements.bin", f("witness.bin"), packed, "--compressed"])
    assert (r.returncode, r.stdout.split()) == (0, ["VERIFIED"]), r.stdout + r.stderr
    vk = gpu.VerificationKey.from_elements(curve, np.fromfile(out / "vk_elements.bin", dtype="<u8").astype(np.uint64))
    proof = np.fromfile(full, dtype="<u8").astype(np.uint64)
    inp = np.fromfile(f("witness.bin"), dtype="<u8", count=24).astype(np.uint64)[12:]
    x, flags = CR.proof_from_stream(curve, packed.read_bytes())
    assert list(vk.verify(proof, inp)) == [0] and list(vk.verify_compressed(x, flags, inp)) == [0]
    flags[2] ^= 1                                                                 # -C
    assert list(vk.verify_compressed(x, flags, inp)) == [2]
    vk.close()
