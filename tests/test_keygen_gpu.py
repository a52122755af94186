"""GPU: Groth16 key generation on the device (mnt753_groth16_generate, `main_hip generate`) against the keys the reference's own
functions made from the same randomness (tests/golden/keygen_mnt{4,6}_{full,cut21}, tools/mint_keygen.sh; tests/test_keygen_cpu.py pins
them to the Python model), the reference's verifier on a proof made with a device-generated key, and the generator's own kernels --
the ABC | Lt combination, the compaction of non-zero scalars and the scatter of their rows -- against tests/keygen_ref.py and numpy.
Every value is an exact field or group element: equal means equal words."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import domain_ref as D
import keygen_ref as K
import oracle_lib as O
from test_groth16_cpu import EXE, NAME, REF

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G1, G2 = 1, 2
PATTERN = 0xA5A5A5A5A5A5A5A5
EINVAL = "rc=-1"
W = 8                      # explicit window width of the tests: tables of a few hundred KB, built in milliseconds at the default tile


def system(gpu, curve, tag, exchange=False):
    """-> (R1cs, Domain) of a fixture's r1cs_in.bin, a and b exchanged on input if asked"""
    ni, m, nc, mats = gpu.read_r1cs_file(os.path.join(K.fixture_dir(curve, tag), "r1cs_in.bin"))
    if exchange:
        mats = [mats[1], mats[0], mats[2]]
    cs = gpu.R1cs(curve, ni, m, nc, mats)
    return cs, gpu.Domain.for_size(curve, cs.domain_size())


def assert_key_equals_fixture(key, curve, tag, tmp_path):
    key.write(str(tmp_path))
    for name in K.QUERY_FILES:
        assert (tmp_path / name).read_bytes() == open(os.path.join(K.fixture_dir(curve, tag), name), "rb").read(), name


@pytest.mark.parametrize("fixture", K.FIXTURES, ids=K.fixture_id)
def test_generated_key_equals_the_reference(gpu, fixture, tmp_path):
    """every output file byte for byte; the densities and the swap decision as the reference's; the domain the reference chose"""
    curve, tag = fixture
    idx = K.index(curve, tag)
    cs, dom = system(gpu, curve, tag)
    assert dom.m == idx["domain_size"] and dom.kind == D.KIND_CODE[K.CLASS_KIND[idx["reference_class"]]]
    t, alpha, beta, delta, g1 = K.randomness(curve, tag)
    key = gpu.generate(cs, dom, t, alpha, beta, delta, g1, g1_window_bits=W, g2_window_bits=W)
    assert (key.non_zero_at, key.non_zero_bt, key.swapped) == (idx["non_zero_At"], idx["non_zero_Bt"], idx["swapped"])
    assert cs.swapped == idx["swapped"]
    assert_key_equals_fixture(key, curve, tag, tmp_path)
    if tag == "cut21":
        # a query goes into a base set as it lies on the device: the same sum as over the fixture's words
        _, _, q = K.split_params(curve, (tmp_path / "params.bin").read_bytes(), cs.num_inputs)
        sc = gpu.synth_scalars(curve, 0x77, cs.m + 1)
        on_dev, on_host = key.bases("B2"), gpu.BaseSet(curve, G2, q["B2"])
        assert on_dev.n == cs.m + 1 and np.array_equal(on_dev.msm(sc), on_host.msm(sc))
        on_dev.close(); on_host.close()
    key.close(); cs.close(); dom.close()


@pytest.mark.parametrize("curve", [0, 1])
def test_default_tables_and_every_compaction_choice(gpu, curve, tmp_path):
    """widths and tiles left to the library (the cache-sized tables); then, at the small width, the G1 queries, the G2 query and both
    without the compaction: the flags change the schedule, never a word"""
    tag = "cut21"
    t, alpha, beta, delta, g1 = K.randomness(curve, tag)
    idx = K.index(curve, tag)
    for k, kw in enumerate((dict(), dict(g1_window_bits=W, g2_window_bits=W, sparse_g1=False), dict(g1_window_bits=W, g2_window_bits=W, sparse_g2=False),
                           dict(g1_window_bits=W, g2_window_bits=W, sparse_g1=False, sparse_g2=False))):
        cs, dom = system(gpu, curve, tag)
        key = gpu.generate(cs, dom, t, alpha, beta, delta, g1, **kw)
        assert (key.non_zero_at, key.non_zero_bt, key.swapped) == (idx["non_zero_At"], idx["non_zero_Bt"], True), kw
        out = tmp_path / str(k)
        assert_key_equals_fixture(key, curve, tag, out)
        key.close(); cs.close(); dom.close()


@pytest.mark.parametrize("curve", [0, 1])
def test_swap_invariance(gpu, curve, tmp_path):
    """`full` with a and b exchanged on input: b now touches 32 variables and a 31, the swap fires, and the key is the key of `full`,
    since the system after the swap is the same.  A second swap on the same object does nothing: 31 < 32."""
    cs, dom = system(gpu, curve, "full", exchange=True)
    t, alpha, beta, delta, g1 = K.randomness(curve, "full")
    key = gpu.generate(cs, dom, t, alpha, beta, delta, g1, g1_window_bits=W, g2_window_bits=W)
    assert key.swapped and cs.swapped
    assert_key_equals_fixture(key, curve, "full", tmp_path)
    assert cs.swap_ab_if_beneficial() is False and cs.swapped
    key.close(); cs.close(); dom.close()


@pytest.mark.parametrize("curve", [0, 1])
def test_swap_reaches_the_witness_evaluation(gpu, curve):
    """after the swap mnt753_r1cs_evaluate gives ca and cb of the swapped system: the fixture's input.bin holds them"""
    tag = "cut21"
    d = K.fixture_dir(curve, tag)
    idx = K.index(curve, tag)
    cs, dom = system(gpu, curve, tag)
    m, dm = cs.m, idx["domain_size"]
    inp = np.fromfile(os.path.join(d, "input.bin"), dtype="<u8").astype(np.uint64).reshape(-1, 12)
    w, want = inp[:m + 1], [inp[m + 1 + k * dm:m + 1 + (k + 1) * dm] for k in range(3)]
    dw = gpu.DeviceBuffer.from_numpy(w)
    outs = [gpu.DeviceBuffer(96 * dm) for _ in range(3)]

    def run():
        cs.evaluate(dw.ptr.value, outs[0].ptr.value, outs[1].ptr.value, outs[2].ptr.value, dm)
        return [o.to_numpy().reshape(dm, 12) for o in outs]

    before, nc = run(), cs.nc
    assert np.array_equal(before[0][:nc], want[1][:nc]) and np.array_equal(before[1][:nc], want[0][:nc])     # as given: a and b the other way round
    assert not np.array_equal(want[0][:nc], want[1][:nc])
    assert cs.swap_ab_if_beneficial() is True
    after = run()
    for got, exp in zip(after, want):
        assert np.array_equal(got, exp)
    cs.close(); dom.close()


def cli(args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True)


@pytest.mark.parametrize("curve", [0, 1])
def test_the_reference_verifier_accepts_a_proof_made_with_a_generated_key(gpu, curve, tmp_path):
    """main_hip generate -> compute-r1cs (the generated params.bin and r1cs.bin, the fixture's witness) -> complete (the generated
    keys.bin) -> the reference's verifier on the fixture's vk.txt and input.bin prints VERIFIED.  cut21: d + 1 = 24 = 16 + 8 is a step
    domain -- a libsnark key with d + 1 not a power of two through the reference's verifier.  A key generated with another delta
    proves just as well and is REJECTED (exit 3) against the fixture's verification key."""
    tag = "cut21"
    fdir = K.fixture_dir(curve, tag)
    f = lambda name: os.path.join(fdir, name)
    O.need_ref("ref_groth16")                     # missing = failure on a GPU box (tests/oracle_lib.py)
    rnd = np.fromfile(f("randomness.bin"), dtype="<u8")
    other = rnd.copy(); other[36:48] = rnd[0:12]                       # delta := t
    (tmp_path / "other.bin").write_bytes(other.tobytes())
    verdicts = []
    for name, rand in (("good", f("randomness.bin")), ("other", tmp_path / "other.bin")):
        out = tmp_path / name
        r = cli([NAME[curve], "generate", f("r1cs_in.bin"), out, "--randomness", rand, "--quiet"])
        assert r.returncode == 0, r.stderr
        chal, full = out / "challenge.bin", out / "full.bin"
        r = cli([NAME[curve], "compute-r1cs", out / "params.bin", out / "r1cs.bin", f("witness.bin"), chal])
        assert r.returncode == 0, r.stderr
        r = cli([NAME[curve], "complete", out / "keys.bin", f("witness.bin"), chal, full, "--s-seed", "99"])
        assert r.returncode == 0, r.stderr
        v = subprocess.run([REF, "verify", NAME[curve], fdir, str(full)], capture_output=True, text=True)
        verdicts.append((v.returncode, v.stdout.strip().splitlines()[-1] if v.stdout.strip() else v.stderr))
    for name in K.QUERY_FILES:
        assert (tmp_path / "good" / name).read_bytes() == open(f(name), "rb").read(), name
    assert verdicts[0] == (0, "VERIFIED"), verdicts
    assert verdicts[1] == (3, "REJECTED"), verdicts


def test_main_hip_generate_command_line(gpu, tmp_path):
    """unknown options and a wrong number of paths exit 2 with the usage text; a randomness file of the wrong size or with delta = 0
    writes nothing; without --randomness the scalars come from the operating system, so two keys differ and both are well formed"""
    curve, tag = 0, "cut21"
    f = lambda name: os.path.join(K.fixture_dir(curve, tag), name)
    r = cli([NAME[curve], "generate", f("r1cs_in.bin"), tmp_path / "x", "--no-such-option"])
    assert r.returncode == 2 and "unknown option" in r.stderr
    r = cli([NAME[curve], "generate", f("r1cs_in.bin")])
    assert r.returncode == 2 and "generate" in r.stderr and "pairing" in r.stderr
    rnd = np.fromfile(f("randomness.bin"), dtype="<u8")
    (tmp_path / "short.bin").write_bytes(rnd.tobytes()[:-8])
    r = cli([NAME[curve], "generate", f("r1cs_in.bin"), tmp_path / "y", "--randomness", tmp_path / "short.bin"])
    assert r.returncode == 1 and not (tmp_path / "y").exists(), r.stderr
    zero_delta = rnd.copy(); zero_delta[36:48] = 0
    (tmp_path / "zd.bin").write_bytes(zero_delta.tobytes())
    r = cli([NAME[curve], "generate", f("r1cs_in.bin"), tmp_path / "z", "--randomness", tmp_path / "zd.bin"])
    assert r.returncode == 3 and "delta" in r.stderr and not (tmp_path / "z" / "params.bin").exists(), r.stderr
    keys = []
    for k in range(2):
        out = tmp_path / f"os{k}"
        r = cli([NAME[curve], "generate", f("r1cs_in.bin"), out])
        assert r.returncode == 0 and "exchanged" in r.stdout, r.stderr
        keys.append((out / "keys.bin").read_bytes())
        assert (out / "params.bin").stat().st_size == os.path.getsize(f("params.bin"))
        assert (out / "r1cs.bin").read_bytes() == open(f("r1cs.bin"), "rb").read()
        pts = np.frombuffer(keys[-1], dtype="<u8").astype(np.uint64)
        assert gpu.check_points(curve, G1, pts[:48]) == (0, 0, 0)
    assert keys[0] != keys[1]


@pytest.mark.parametrize("curve", [0, 1])
def test_combination_kernel(gpu, curve):
    """(beta At + alpha Bt + Ct) c_i against the model at lengths 1, 2, 17, 1025 with num_inputs 0, 1 and length - 1: the index where
    c_i changes at the first entry, at the last and on a workgroup edge (num_inputs = 255 and 256 at length 1025 too); entries 0, r - 1
    and sums that wrap; in place on one of the inputs"""
    r = D.MODULUS[curve]
    alpha, beta, dinv = (D.from_wire(curve, gpu.synth_scalars(curve, 0x90 + k, 1))[0] for k in range(3))
    rng = np.random.default_rng(11 + curve)
    pool = D.from_wire(curve, gpu.synth_scalars(curve, 0x99, 64))
    special = [0, r - 1, 1, r - 2, (r + 1) // 2]
    for n in (1, 2, 17, 1025):
        vecs = []
        for k in range(3):
            v = [pool[int(j)] for j in rng.integers(0, 64, size=n)]
            for i in range(0, n, 3):
                v[i] = special[(i // 3 + k) % len(special)]
            vecs.append(v)
        vecs[0][0], vecs[1][0], vecs[2][0] = r - 1, r - 1, r - 1                       # every term wraps
        if n > 1:
            vecs[0][n - 1], vecs[1][n - 1], vecs[2][n - 1] = 0, 0, 0                   # a zero entry stays zero
        bufs = [gpu.DeviceBuffer.from_numpy(D.to_wire(curve, v)) for v in vecs]
        out = gpu.DeviceBuffer(96 * n)
        for ni in sorted({0, min(1, n - 1), n - 1} | ({255, 256} if n > 256 else set())):
            want = D.to_wire(curve, K.combine(curve, vecs[0], vecs[1], vecs[2], ni, alpha, beta, dinv))
            gpu.keygen_combine(curve, bufs[0].ptr.value, bufs[1].ptr.value, bufs[2].ptr.value, n, ni, D.to_wire(curve, [beta])[0],
                               D.to_wire(curve, [alpha])[0], D.to_wire(curve, [dinv])[0], out.ptr.value)
            assert np.array_equal(out.to_numpy().reshape(n, 12), want), (n, ni)
        inplace = gpu.DeviceBuffer.from_numpy(D.to_wire(curve, vecs[2]))
        gpu.keygen_combine(curve, bufs[0].ptr.value, bufs[1].ptr.value, inplace.ptr.value, n, 0, D.to_wire(curve, [beta])[0],
                           D.to_wire(curve, [alpha])[0], D.to_wire(curve, [dinv])[0], inplace.ptr.value)
        assert np.array_equal(inplace.to_numpy().reshape(n, 12), D.to_wire(curve, K.combine(curve, vecs[0], vecs[1], vecs[2], 0, alpha, beta, dinv))), n
        for b in bufs + [out, inplace]:
            b.close()
    big = np.full(12, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)                              # a factor >= r is refused
    one = gpu.DeviceBuffer.from_numpy(D.to_wire(curve, [1]))
    with pytest.raises(gpu.Mnt753Error, match=EINVAL):
        gpu.keygen_combine(curve, one.ptr.value, one.ptr.value, one.ptr.value, 1, 0, big, big, big, one.ptr.value)
    one.close()


LENGTHS = (1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 4097)


def zero_masks(n):
    """name -> boolean mask of the ZERO entries"""
    idx = np.arange(n)
    run = (idx >= 60) & (idx < 260)                    # one zero run over a wave edge (64) and a workgroup edge (256), cut to n
    if n <= 60:
        run = idx >= n // 2                            # shorter vectors: the run is their upper half
    return {"all zero": np.ones(n, bool), "none zero": np.zeros(n, bool), "alternating": idx % 2 == 0, "only the first non-zero": idx != 0,
            "only the last non-zero": idx != n - 1, "one zero run": run}


@pytest.mark.parametrize("n", LENGTHS)
def test_compaction_and_scatter(gpu, n):
    """indices = numpy's flatnonzero (strictly increasing), the count, the compacted elements in order; the scattered rows have zero
    words exactly where the input was zero.  Values that differ from zero in the top word only or in the bottom word only count."""
    base = gpu.synth_scalars(0, 0xC0, n)
    assert base.any(axis=1).all()
    variants = {"synthetic": base, "top word only": np.zeros((n, 12), np.uint64), "bottom word only": np.zeros((n, 12), np.uint64)}
    variants["top word only"][:, 11] = 1
    variants["bottom word only"][:, 0] = np.arange(1, n + 1, dtype=np.uint64)
    row_words = 48
    comp, index = gpu.DeviceBuffer(96 * n), gpu.DeviceBuffer(4 * n)
    rows_host = (np.arange(n * row_words, dtype=np.uint64) + 1).reshape(n, row_words)
    rows, out = gpu.DeviceBuffer.from_numpy(rows_host), gpu.DeviceBuffer(8 * row_words * n)
    for vname, values in variants.items():
        for mname, zero in zero_masks(n).items():
            v = values.copy()
            v[zero] = 0
            want = np.flatnonzero(v.any(axis=1))
            dv = gpu.DeviceBuffer.from_numpy(v)
            gpu.lib().mnt753_dev_memset(comp.ptr, 0xEE, 96 * n)
            gpu.lib().mnt753_dev_memset(index.ptr, 0xEE, 4 * n)
            assert gpu.compact_nonzero(dv.ptr.value, n) == len(want), (vname, mname)             # the count alone
            count = gpu.compact_nonzero(dv.ptr.value, n, comp.ptr.value, index.ptr.value)
            assert count == len(want), (vname, mname)
            got_idx = index.to_numpy(np.uint32)
            assert np.array_equal(got_idx[:count], want) and (got_idx[count:] == 0xEEEEEEEE).all(), (vname, mname)
            got = comp.to_numpy().reshape(n, 12)
            assert np.array_equal(got[:count], v[want]) and (got[count:] == 0xEEEEEEEEEEEEEEEE).all(), (vname, mname)
            gpu.lib().mnt753_dev_memset(out.ptr, 0xEE, 8 * row_words * n)
            gpu.scatter_rows(rows.ptr.value, index.ptr.value, count, row_words, out.ptr.value, n)
            gpu.lib().mnt753_sync(None)
            sc = out.to_numpy().reshape(n, row_words)
            assert np.array_equal(sc[want], rows_host[:count]) and not sc[zero].any(), (vname, mname)
            assert (sc.any(axis=1) == ~zero).all(), (vname, mname)
            dv.close()
    for b in (comp, index, rows, out):
        b.close()


@pytest.mark.parametrize("curve,group", [(0, G1), (0, G2), (1, G1), (1, G2)])
def test_batch_exp_through_compaction_equals_batch_exp(gpu, curve, group):
    """n = 65 (two waves), zeros at both ends, in a run and scattered; with and without a coefficient; all zero (nothing is walked,
    the output is zeroed) and none zero (the vector as it lies)"""
    n = 65
    aw = gpu.affine_words(curve, group)
    fb = gpu.FixedBase(curve, group, gpu.group_generator(curve, group), window_bits=W)
    coeff = gpu.synth_scalars(curve, 0xD1, 1)[0]
    base = gpu.synth_scalars(curve, 0xD0, n)
    some = base.copy()
    some[[0, 1, 5, 30, 31, 32, 33, 63, 64]] = 0
    for name, v in (("some", some), ("all zero", np.zeros_like(base)), ("none zero", base)):
        dv = gpu.DeviceBuffer.from_numpy(v)
        for c in (None, coeff):
            want = fb.batch_exp(v, coeff=c)
            out = gpu.DeviceBuffer.from_numpy(np.full(n * aw, PATTERN, dtype=np.uint64))
            count = fb.batch_exp_sparse(dv.ptr.value, n, out.ptr.value, coeff=c)
            assert count == int(v.any(axis=1).sum()), name
            got = out.to_numpy().reshape(n, aw)
            assert np.array_equal(got, want), (name, c is not None)
            assert (got.any(axis=1) == v.any(axis=1)).all(), name
            out.close()
        dv.close()
    fb.close()


def raw_generate(gpu, cs, dom, t, alpha, beta, delta, g1, bufs, singles):
    """mnt753_groth16_generate into the caller's buffers -> return code"""
    api = gpu.api
    u64p = C.POINTER(C.c_uint64)
    out = api.KeygenOut(*[b.ptr.value for b in bufs], *[s.ctypes.data for s in singles])
    opts = api.KeygenOpts(W, W, 0, 0, 0, 0)
    rep = api.KeygenReport()
    args = [np.ascontiguousarray(x, dtype=np.uint64) for x in (t, alpha, beta, delta, g1)]
    return gpu.lib().mnt753_groth16_generate(cs._h, dom._h, *[a.ctypes.data_as(u64p) for a in args], C.byref(opts), C.byref(out), C.byref(rep), None)


@pytest.mark.parametrize("curve", [0, 1])
def test_refusals_leave_everything_untouched(gpu, curve):
    """alpha, beta or delta zero; t, alpha, beta or delta >= r; t in the domain (t = 1: Z(t) = 0); the G1 generator the identity, off
    the curve or not canonical; a domain that is too small or of the other curve: MNT753_EINVAL, every output buffer keeps its
    pattern, and the system is not swapped.  The same buffers are then written by a good call."""
    tag = "cut21"
    cs, dom = system(gpu, curve, tag)
    t, alpha, beta, delta, g1 = K.randomness(curve, tag)
    w1, w2 = gpu.affine_words(curve, G1), gpu.affine_words(curve, G2)
    m, ni, dm = cs.m, cs.num_inputs, dom.m
    sizes = [w1 * (m + 1), w1 * (m + 1), w2 * (m + 1), w1 * (m - ni), w1 * (dm - 1), w1 * (ni + 1)]
    fills = [np.full(s, PATTERN, dtype=np.uint64) for s in sizes]
    bufs = [gpu.DeviceBuffer.from_numpy(f) for f in fills]
    singles = [np.full(w, PATTERN, dtype=np.uint64) for w in (w1, w1, w2, w1, w2)]
    zero, big = np.zeros(12, dtype=np.uint64), np.full(12, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    r_w = D.ints_to_words([D.MODULUS[curve]])[0]
    one = gpu.api.mont_one(curve)
    off_curve = g1.copy(); off_curve[0] ^= 1
    not_canonical = g1.copy(); not_canonical[:12] = 0xFFFFFFFFFFFFFFFF
    small, other = gpu.Domain(curve, 16), gpu.Domain(1 - curve, 32)
    cases = {"alpha = 0": (dom, t, zero, beta, delta, g1), "beta = 0": (dom, t, alpha, zero, delta, g1), "delta = 0": (dom, t, alpha, beta, zero, g1),
             "t >= r": (dom, big, alpha, beta, delta, g1), "alpha = r": (dom, t, r_w, beta, delta, g1), "beta >= r": (dom, t, alpha, big, delta, g1),
             "delta = r": (dom, t, alpha, beta, r_w, g1), "t in the domain": (dom, one, alpha, beta, delta, g1),
             "generator = identity": (dom, t, alpha, beta, delta, np.zeros(24, dtype=np.uint64)), "generator off curve": (dom, t, alpha, beta, delta, off_curve),
             "generator not canonical": (dom, t, alpha, beta, delta, not_canonical), "domain too small": (small, t, alpha, beta, delta, g1),
             "domain of the other curve": (other, t, alpha, beta, delta, g1)}
    for name, (d, *rest) in cases.items():
        assert raw_generate(gpu, cs, d, *rest, bufs, singles) == -1, name
        assert gpu.lib().mnt753_last_error(), name
    gpu.lib().mnt753_sync(None)
    for b, f in zip(bufs, fills):
        assert np.array_equal(b.to_numpy(), f)
    assert all((s == PATTERN).all() for s in singles) and not cs.swapped
    assert raw_generate(gpu, cs, dom, t, alpha, beta, delta, g1, bufs, singles) == 0
    params = np.fromfile(os.path.join(K.fixture_dir(curve, tag), "params.bin"), dtype="<u8").astype(np.uint64)[2:]
    assert np.array_equal(np.concatenate([b.to_numpy() for b in bufs[:5]]), params) and cs.swapped
    keys = np.fromfile(os.path.join(K.fixture_dir(curve, tag), "keys.bin"), dtype="<u8").astype(np.uint64)
    assert np.array_equal(np.concatenate(singles), keys)
    for x in bufs + [cs, dom, small, other]:
        x.close()


ON_OTHER_DEVICE = r'''
import json, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import ctypes as C
import numpy as np
from __graft_entry__ import load_package
import keygen_ref as K
pkg = load_package()
L = pkg.api.lib()
assert L.mnt753_init_devices(2) == 0, L.mnt753_last_error().decode()
curve, tag = 0, "cut21"
ni, m, nc, mats = pkg.read_r1cs_file(K.fixture_dir(curve, tag) + "/r1cs_in.bin")
assert L.mnt753_set_device(0) == 0
cs = pkg.R1cs(curve, ni, m, nc, mats)
assert L.mnt753_set_device(1) == 0
dom = pkg.Domain.for_size(curve, cs.domain_size())         # lives on logical device 1
assert L.mnt753_set_device(0) == 0
t, alpha, beta, delta, g1 = K.randomness(curve, tag)
out = {"domain_device": int(L.mnt753_domain_device(dom._h))}
try:
    pkg.generate(cs, dom, t, alpha, beta, delta, g1, g1_window_bits=8, g2_window_bits=8)
    out["error"] = None
except pkg.Mnt753Error as e:
    out["error"] = str(e)
out["swapped"] = cs.swapped
print(json.dumps(out), flush=True)
'''


def test_a_domain_on_another_device_is_refused(gpu):
    """Under MNT753_SHARE_DEVICE=1 two logical devices map onto the one GPU: a system on device 0 and a domain on device 1 are refused
    with MNT753_EINVAL before the system is swapped.  A fresh child process: the devices are set up once per process."""
    r = subprocess.run([sys.executable, "-c", ON_OTHER_DEVICE % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}], capture_output=True, text=True,
                       timeout=300, env=dict(os.environ, MNT753_SHARE_DEVICE="1"))
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["domain_device"] == 1 and out["error"] and EINVAL in out["error"] and "different devices" in out["error"], out
    assert out["swapped"] is False
