"""CPU: compressed points (include/mnt753_hip.h "compressed points") as far as they go without a device.

* tests/compress_ref.py -- compression, the decompression rules and libff's stream records in Python integers -- against
  tests/golden/compress/, minted by libff with point compression ON (tools/mint_compress.sh): the GPU tests stand on it.
* mnt753_points_to_stream / mnt753_points_from_stream (host code of the product) against the same fixture.
* tools/host_sqrt_check.cpp: the device's own square root (csrc/fp_sqrt.hip.h) through the one-lane fields under g++, plain and with
  -fsanitize=address,undefined (a stand-alone program).
* the ABI: symbols declared, exported and in the sanitizer stub; argument errors and the no-device answers; the CLI without a GPU and
  through the `make asan` stub binary."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest

import compress_ref as CR
import oracle_lib as O
from test_abi_cpu import exported, has_gpu, header_symbols
from test_validate_cpu import EXE, NAME, asan, g16, run_san  # noqa: F401  (asan: the module-scoped fixture that runs `make asan`)

ROOT = O.ROOT
FIX = os.path.join(ROOT, "tests", "golden", "compress")
NEW = ("mnt753_compressed_words", "mnt753_compress_points", "mnt753_decompress_points", "mnt753_groth16_verify_compressed",
       "mnt753_points_to_stream", "mnt753_points_from_stream")
HOOKS = ("mnt753_test_field_sqrt", "mnt753_test_field_sqrt_window")
N_POINTS, IDENTITY_AT = 16, 5


def group_dir(curve, group):
    return os.path.join(FIX, f"mnt{4 if curve == 0 else 6}_g{group}")


def fixture(curve, group):
    """(points [16, 2 Wx] uint64, stream bytes)"""
    d = group_dir(curve, group)
    pts = np.fromfile(os.path.join(d, "points.bin"), dtype=np.uint64).reshape(N_POINTS, -1)
    return pts, open(os.path.join(d, "stream.bin"), "rb").read()


def proof_fixture(curve):
    """(the affine proof of tests/golden/g16_mnt*/full.bin, its compressed stream)"""
    return np.fromfile(g16(curve, "full.bin"), dtype=np.uint64), open(os.path.join(FIX, f"mnt{4 if curve == 0 else 6}", "proof_stream.bin"), "rb").read()


def test_fixture_manifest():
    """tests/golden/compress/SHA256SUMS lists every file of the fixture with its digest; a few KB in all"""
    listed = {}
    for line in open(os.path.join(FIX, "SHA256SUMS")):
        digest, name = line.split()
        listed[name] = digest
    found = sorted(os.path.relpath(os.path.join(d, f), FIX) for d, _, fs in os.walk(FIX) for f in fs if f != "SHA256SUMS")
    assert found == sorted(listed) and len(found) == 10
    for name in found:
        assert hashlib.sha256(open(os.path.join(FIX, name), "rb").read()).hexdigest() == listed[name], name
    assert sum(os.path.getsize(os.path.join(FIX, name)) for name in found) < 40000


@pytest.mark.parametrize("curve,group", CR.GROUPS)
def test_reference_against_libff(curve, group):
    pts, stream = fixture(curve, group)
    assert pts.shape == (N_POINTS, 2 * CR.x_words(curve, group)) and len(stream) == N_POINTS * CR.record_bytes(curve, group)
    assert not pts[IDENTITY_AT].any() and all(pts[i].any() for i in range(N_POINTS) if i != IDENTITY_AT)
    x, flags = CR.compress(curve, group, pts)
    assert flags[IDENTITY_AT] == CR.FLAG_IDENTITY and {0, 1} <= set(int(f) for f in flags)          # both parities are there
    assert CR.to_stream(curve, group, x, flags) == stream
    sx, sf = CR.from_stream(curve, group, stream)
    assert np.array_equal(sx, x) and np.array_equal(sf, flags)
    back, rep = CR.decompress(curve, group, sx, sf)
    assert rep == (0, 0, CR.BAD_NONE) and np.array_equal(back, pts)
    # the other flag gives the other root, and nothing else changes
    other, rep = CR.decompress(curve, group, sx, sf ^ np.where(sf == CR.FLAG_IDENTITY, 0, 1).astype(np.uint8))
    cv = CR.CURVES[curve]
    for i in range(N_POINTS):
        p, q = CR.DP.from_words(curve, group, pts[i]), CR.DP.from_words(curve, group, other[i])
        assert q == cv.neg(p)


@pytest.mark.parametrize("curve", [0, 1])
def test_reference_proof_stream_against_libff(curve):
    proof, stream = proof_fixture(curve)
    assert len(stream) == (390, 486)[curve]
    x, flags = CR.compress_proofs(curve, proof)
    assert CR.proof_to_stream(curve, x[0], flags[0]) == stream
    sx, sf = CR.proof_from_stream(curve, stream)
    assert np.array_equal(sx, x[0]) and np.array_equal(sf, flags[0])
    at, parts = 0, []
    for k, (group, _, _) in enumerate(CR.proof_parts(curve)):
        wx = CR.x_words(curve, group)
        pts, rep = CR.decompress(curve, group, sx[at:at + wx], sf[k:k + 1])
        assert rep == (0, 0, CR.BAD_NONE)
        parts.append(pts.reshape(-1))
        at += wx
    assert np.array_equal(np.concatenate(parts), proof)


@pytest.mark.parametrize("curve,group", CR.GROUPS)
def test_reference_rules(curve, group):
    """precedence per point: non-canonical before the identity before off-curve; bad points are zero words"""
    cv = CR.CURVES[curve]
    wx = CR.x_words(curve, group)
    good_x, good_f = CR.compress_point(curve, group, cv.gen(group))
    bad_x = [int(v) for v in CR.non_liftable_words(curve, group)]
    q_words = [(cv.q >> (64 * i)) & (2 ** 64 - 1) for i in range(12)] + [0] * (wx - 12)
    ones = [2 ** 64 - 1] * wx
    rows = [(good_x, good_f, CR.BAD_NONE), (bad_x, 0, CR.BAD_OFF_CURVE), (bad_x, 1, CR.BAD_OFF_CURVE), (bad_x, 2, CR.BAD_NONE), (bad_x, 4, CR.BAD_NONCANONICAL),
            (q_words, 0, CR.BAD_NONCANONICAL), (q_words, 2, CR.BAD_NONCANONICAL), (ones, 0, CR.BAD_NONCANONICAL), (good_x, 6, CR.BAD_NONCANONICAL),
            (good_x, 2, CR.BAD_NONE), (good_x, 0x80 | good_f, CR.BAD_NONCANONICAL)]
    x = np.array([r[0] for r in rows], dtype=np.uint64)
    f = np.array([r[1] for r in rows], dtype=np.uint8)
    pts, rep = CR.decompress(curve, group, x, f)
    bad = [i for i, r in enumerate(rows) if r[2] != CR.BAD_NONE]
    assert rep == (len(bad), bad[0], rows[bad[0]][2])
    assert np.array_equal(pts[0], CR.DP.to_words(curve, group, cv.gen(group))) and not pts[1:].any()
    for i, r in enumerate(rows):
        assert CR.decompress_point(curve, group, r[0], r[1])[1] == r[2], i


# ---- the product's stream codec (host code, no device) --------------------------------------------------------------------------------
@pytest.mark.parametrize("curve,group", CR.GROUPS)
def test_product_streams_against_libff(pkg, curve, group):
    pts, stream = fixture(curve, group)
    x, flags = CR.compress(curve, group, pts)
    assert pkg.compressed_words(curve, group) == CR.x_words(curve, group)
    assert pkg.points_to_stream(curve, group, x, flags) == stream
    sx, sf = pkg.points_from_stream(curve, group, stream)
    assert np.array_equal(sx, x) and np.array_equal(sf, flags)
    rec = CR.record_bytes(curve, group)
    at = IDENTITY_AT * rec
    assert stream[at:at + 1] == b"1" and stream[at + rec - 1:at + rec] == b"1" and not any(stream[at + 1:at + rec - 1])
    # both parity bytes are accepted for the identity, and whatever its x holds it comes back as x = 0, flag 2
    for par in (b"0", b"1"):
        alt = bytearray(stream)
        alt[at + rec - 1:at + rec] = par
        alt[at + 1:at + 9] = b"\x07" * 8
        ax, af = pkg.points_from_stream(curve, group, bytes(alt))
        assert np.array_equal(ax, x) and np.array_equal(af, flags)
    # a byte '2' in either flag position, a buffer one byte short
    for pos in (0, rec - 1, 3 * rec, 4 * rec - 1):
        alt = bytearray(stream)
        alt[pos:pos + 1] = b"2"
        with pytest.raises(pkg.Mnt753Error, match="rc=-1"):
            pkg.points_from_stream(curve, group, bytes(alt))
    with pytest.raises(pkg.Mnt753Error, match="rc=-1"):
        pkg.points_from_stream(curve, group, stream[:-1], n=N_POINTS)
    assert len(pkg.points_from_stream(curve, group, stream[:-1])[1]) == N_POINTS - 1     # n from the buffer: whole records only
    with pytest.raises(pkg.Mnt753Error, match="rc=-1"):
        pkg.points_to_stream(curve, group, x, flags | np.uint8(4))
    assert pkg.points_to_stream(curve, group, x[:0], flags[:0]) == b""


@pytest.mark.parametrize("curve", [0, 1])
def test_product_proof_stream_against_libff(pkg, curve):
    proof, stream = proof_fixture(curve)
    x, flags = CR.compress_proofs(curve, proof)
    out, at = b"", 0
    for k, (group, _, _) in enumerate(CR.proof_parts(curve)):
        wx = CR.x_words(curve, group)
        out += pkg.points_to_stream(curve, group, x[0, at:at + wx], flags[0, k:k + 1])
        at += wx
    assert out == stream


def test_stream_argument_errors(pkg):
    L = pkg.lib()
    buf = np.zeros(64, dtype=np.uint64)
    p = ctypes.c_void_p(buf.ctypes.data)
    ln = ctypes.c_size_t()
    EINVAL = -1
    assert [pkg.compressed_words(c, g) for c in (0, 1) for g in (1, 2)] == [12, 24, 12, 36]
    assert pkg.compressed_words(2, 1) == 0 and pkg.compressed_words(0, 3) == 0
    assert L.mnt753_points_to_stream(2, 1, p, p, 1, None, 0, ctypes.byref(ln)) == EINVAL
    assert L.mnt753_points_to_stream(0, 1, None, p, 1, None, 0, ctypes.byref(ln)) == EINVAL
    assert L.mnt753_points_to_stream(0, 1, p, p, 1, None, 0, None) == EINVAL
    assert L.mnt753_points_to_stream(0, 1, p, p, 2, None, 0, ctypes.byref(ln)) == 0 and ln.value == 196          # the size alone
    assert L.mnt753_points_to_stream(0, 1, p, p, 2, p, 195, ctypes.byref(ln)) == EINVAL                            # too small
    assert L.mnt753_points_from_stream(0, 0, p, 98, 1, p, p) == EINVAL
    assert L.mnt753_points_from_stream(0, 1, None, 98, 1, p, p) == EINVAL
    assert L.mnt753_points_from_stream(0, 1, p, 0, 0, None, None) == 0


# ---- the device's own square root on the host -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_sqrt(tmp_path_factory):
    exe = tmp_path_factory.mktemp("host_sqrt") / "host_sqrt_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tools", "host_sqrt_check.cpp")], check=True, timeout=600)
    return str(exe)


def test_device_square_root_on_the_host(host_sqrt):
    out = subprocess.run([host_sqrt], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0 and "ALL OK" in out.stdout and out.stdout.count(": OK") == 12, out.stdout + out.stderr


def test_device_square_root_on_the_host_under_sanitizers():
    """`make asan` also builds tools/host_sqrt_check.cpp with -fsanitize=address,undefined: a stand-alone program, run directly"""
    r = subprocess.run(["make", "build/san/host_sqrt_check_asan"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    out = subprocess.run([os.path.join(ROOT, "build", "san", "host_sqrt_check_asan")], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0 and "ALL OK" in out.stdout and "runtime error" not in out.stderr, out.stdout + out.stderr


def test_square_root_constants_are_generated():
    """csrc/mnt753_sqrt_constants.h is what tools/gen_constants.py writes from the two moduli, and the 2-adicities are the four of the issue"""
    import gen_constants as GC
    import mnt753_params as P
    got = [GC.sqrt_constants(q, deg, nr)["s"] for q, deg, nr in ((P.MOD_B, 1, 0), (P.MOD_A, 1, 0), (P.MOD_B, 2, 13), (P.MOD_A, 3, 11))]
    assert got == [15, 30, 16, 30]
    text = open(os.path.join(ROOT, "snark-challenge-prover-reference_amd", "csrc", "mnt753_sqrt_constants.h")).read()
    for q, deg, nr in ((P.MOD_B, 1, 0), (P.MOD_A, 3, 11)):
        c = GC.sqrt_constants(q, deg, nr)
        assert GC.arr(GC.limbs(c["e"], GC.SQRT_WORDS, 32)) in text
        for v in c["zt"]:
            assert GC.arr(GC.limbs(v * (1 << GC.RP_BITS) % q, GC.NL, GC.LB), 7) in text


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_stubbed(pkg):
    syms = header_symbols()
    prod = exported(pkg.lib_path())
    stub = open(os.path.join(ROOT, "tools", "stub_abi", "stub_mnt753.cpp")).read()
    for s in NEW:
        assert s in syms and s in prod and f" {s}(" in stub, s
    hooks = header_symbols("mnt753_hip_test.h")
    for s in HOOKS:
        assert s in hooks and s in exported(pkg.api.test_lib_path()) and s not in prod, s
    for name in ("compressed_words", "compress_points", "decompress_points", "points_to_stream", "points_from_stream"):
        assert callable(getattr(pkg, name))
    assert callable(pkg.VerificationKey.verify_compressed)


def test_argument_errors(pkg):
    """null pointers and bad ids are MNT753_EINVAL, with or without a device"""
    L = pkg.lib()
    rep = pkg.CheckReport()
    buf = np.zeros(144, dtype=np.uint64)
    p = ctypes.c_void_p(buf.ctypes.data)
    EINVAL = -1
    assert L.mnt753_compress_points(2, 1, p, 0, 1, p, p, None) == EINVAL
    assert L.mnt753_compress_points(0, 0, p, 0, 1, p, p, None) == EINVAL
    assert L.mnt753_compress_points(0, 1, None, 0, 1, p, p, None) == EINVAL
    assert L.mnt753_compress_points(0, 1, p, 0, 1, None, p, None) == EINVAL
    assert L.mnt753_compress_points(0, 1, p, 0, 1, p, None, None) == EINVAL
    assert L.mnt753_decompress_points(0, 3, p, p, 0, 1, p, ctypes.byref(rep), None) == EINVAL
    assert L.mnt753_decompress_points(0, 1, None, p, 0, 1, p, ctypes.byref(rep), None) == EINVAL
    assert L.mnt753_decompress_points(0, 1, p, None, 0, 1, p, ctypes.byref(rep), None) == EINVAL
    assert L.mnt753_decompress_points(0, 1, p, p, 0, 1, None, ctypes.byref(rep), None) == EINVAL
    assert L.mnt753_decompress_points(0, 1, p, p, 0, 1, p, None, None) == EINVAL
    assert L.mnt753_decompress_points(0, 1, None, None, 0, 0, None, None, None) == EINVAL          # the report is needed at n = 0 too
    assert L.mnt753_groth16_verify_compressed(None, p, p, p, 1, 0, 0, p, None) == EINVAL
    assert L.mnt753_groth16_verify_compressed(None, None, None, None, 0, 0, 0, None, None) == EINVAL


@pytest.mark.skipif(has_gpu(), reason="checks the no-device behaviour")
def test_calls_refuse_without_a_device(pkg):
    L = pkg.lib()
    rep = pkg.CheckReport()
    buf = np.zeros(144, dtype=np.uint64)
    p = ctypes.c_void_p(buf.ctypes.data)
    ENODEV = -2
    for n in (0, 1):
        assert L.mnt753_compress_points(0, 1, p, 0, n, p, p, None) == ENODEV
        assert L.mnt753_decompress_points(1, 2, p, p, 0, n, p, ctypes.byref(rep), None) == ENODEV
    assert b"no HIP device" in L.mnt753_last_error()
    with pytest.raises(pkg.Mnt753Error):
        pkg.compress_points(0, 1, np.zeros((1, 24), dtype=np.uint64))


@pytest.mark.skipif(has_gpu(), reason="checks the no-device behaviour")
@pytest.mark.parametrize("curve", [0, 1])
def test_cli_fails_loudly_without_gpu(curve, tmp_path):
    stream = os.path.join(FIX, f"mnt{4 if curve == 0 else 6}", "proof_stream.bin")
    out = tmp_path / "o.bin"
    for args in ([NAME[curve], "compress-proof", g16(curve, "full.bin"), str(out)], [NAME[curve], "decompress-proof", stream, str(out)]):
        r = subprocess.run([EXE] + args, capture_output=True, text=True)
        assert r.returncode == 1 and "no HIP device" in r.stderr, (args, r.returncode, r.stderr)
        assert not out.exists()
    import keygen_ref as K
    r = subprocess.run([EXE, NAME[curve], "verify", g16_vk(curve, K), g16(curve, "input.bin"), stream, "--compressed"], capture_output=True, text=True)
    assert r.returncode == 1 and "no HIP device" in r.stderr and r.stdout == ""


def g16_vk(curve, K):
    """a vk_elements.bin to verify against (the CLI stops at the device before it looks at what the key is for)"""
    return os.path.join(K.fixture_dir(curve, "full"), "vk_elements.bin")


def test_cli_usage(tmp_path):
    """unknown options and wrong word counts are refused with exit 2, as everywhere; a file that is no stream with 3"""
    full, out = g16(0, "full.bin"), str(tmp_path / "o.bin")
    for args in (["MNT4753", "compress-proof"], ["MNT4753", "compress-proof", full], ["MNT4753", "compress-proof", full, out, out],
                 ["MNT4753", "compress-proof", full, out, "--frobnicate"], ["MNT4753", "decompress-proof", full, out, "--compressed"],
                 ["BN128", "compress-proof", full, out], ["MNT4753", "vk", full, out, "--compressed"]):
        r = subprocess.run([EXE] + args, capture_output=True, text=True)
        assert r.returncode == 2, (args, r.returncode, r.stderr)
    r = subprocess.run([EXE, "MNT4753", "decompress-proof", full, out], capture_output=True, text=True)       # 768 bytes: not a stream
    assert r.returncode == 3 and "not a compressed proof" in r.stderr and not os.path.exists(out)
    bad = tmp_path / "bad.bin"
    stream = bytearray(open(os.path.join(FIX, "mnt4", "proof_stream.bin"), "rb").read())
    stream[98:99] = b"2"                                                                                      # the is-zero byte of B
    bad.write_bytes(bytes(stream))
    r = subprocess.run([EXE, "MNT4753", "decompress-proof", str(bad), out], capture_output=True, text=True)
    assert r.returncode == 3 and ": B: " in r.stderr and not os.path.exists(out)


@pytest.mark.parametrize("curve", [0, 1])
def test_cli_clean_under_asan(asan, curve, tmp_path):
    """compress-proof, decompress-proof and verify --compressed through the stub of the C ABI (no arithmetic: the stream codec is the
    product's own, the points are not)"""
    import keygen_ref as K
    name = NAME[curve]
    stream = os.path.join(FIX, f"mnt{4 if curve == 0 else 6}", "proof_stream.bin")
    packed, back = tmp_path / "p.bin", tmp_path / "b.bin"
    run_san(asan, [name, "compress-proof", g16(curve, "full.bin"), str(packed)], 0)
    assert packed.stat().st_size == (390, 486)[curve]
    run_san(asan, [name, "decompress-proof", str(packed), str(back)], 0)
    assert back.stat().st_size == (768, 960)[curve]
    back.unlink()
    r = run_san(asan, [name, "decompress-proof", str(packed), str(back)], 3, {"MNT753_STUB_BAD_POINT": "0"})
    assert "A: off curve" in r.stderr and not back.exists()
    vk = g16_vk(curve, K)
    r = run_san(asan, [name, "verify", vk, g16(curve, "input.bin"), stream, stream, "--compressed"], 0)
    assert r.stdout.split() == ["VERIFIED", "VERIFIED"]
    r = run_san(asan, [name, "verify", vk, g16(curve, "input.bin"), stream, "--compressed", "--check-subgroup"], 3, {"MNT753_STUB_BAD_B": "0"})
    assert "REJECTED (B not in the subgroup)" in r.stdout
    ident = bytearray(open(stream, "rb").read())
    ident[0:1] = b"1"                                                                                         # A: the identity
    (tmp_path / "i.bin").write_bytes(bytes(ident))
    r = run_san(asan, [name, "verify", vk, g16(curve, "input.bin"), str(tmp_path / "i.bin"), "--compressed"], 3)
    assert r.stdout.strip() == "REJECTED (malformed)"
    run_san(asan, [name, "verify", vk, g16(curve, "input.bin"), stream, "--compressed", "--fold"], 2)
