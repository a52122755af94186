"""GPU: the reductions over Fr (mnt753_vec_dot, mnt753_poly_eval, mnt753_domain_interp_at) and the spot check of compute_H built on
them (mnt753_h_check, mnt753_compute_h_checked, `main_hip --check-h`), bit for bit against Python integers (tests/hcheck_ref.py,
which tests/test_hcheck_cpu.py exercises on its own).  Every t is fixed by a seed and the model predicts each verdict for that t."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import domain_ref as D
import golden_io as G
import hcheck_ref as H
import keygen_ref as K
import qap_ref as Q
from test_groth16_cpu import EXE, NAME, fx

pytestmark = pytest.mark.gpu

PATTERN = 0xA5A5A5A5A5A5A5A5
SIZES = [0, 1, 63, 64, 65, 255, 256, 257]
CAP = 2                                   # blocks of the capped launches: one coverage is 512 elements / 8192 coefficients
BIG = 3 * CAP * 256 * 16 + 16 * 5 + 3     # about three coverages of the capped polynomial grid plus an odd remainder
POOL_N = (1 << 16) + 32                   # the largest domain below plus the offsets of the windows taken from the pool
_POOL = {}


def pool(gpu, curve):
    """POOL_N seeded random elements of Fr as (wire array, integers, device buffer), made once per curve and never written"""
    if curve not in _POOL:
        w = gpu.synth_scalars(curve, 0x4843 + curve, POOL_N)
        _POOL[curve] = (w, D.from_wire(curve, w), gpu.DeviceBuffer.from_numpy(w))
    return _POOL[curve]


def dev(gpu, curve, ints):
    return gpu.DeviceBuffer.from_numpy(D.to_wire(curve, ints) if len(ints) else np.zeros((1, 12), dtype=np.uint64))


def capped(gpu, curve, op, a_ptr, b_ptr, n, t_w, blocks):
    out = np.zeros(12, dtype=np.uint64)
    pt = None if t_w is None else np.ascontiguousarray(t_w, dtype=np.uint64).ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    rc = gpu.test_lib().mnt753_test_reduce_capped(curve, op, ctypes.c_void_p(a_ptr), ctypes.c_void_p(b_ptr), n, pt, blocks,
                                                  out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)))
    assert rc == 0, gpu.lib().mnt753_last_error()
    return out


def as_int(curve, words):
    return H.unwire1(curve, words)


@pytest.mark.parametrize("curve", [0, 1])
def test_vec_dot_sizes_and_grid_trips(gpu, curve):
    """seeded random vectors at the sizes around a wave and a block, and under a cap of 2 blocks: exactly one coverage of the grid
    (512), one fewer, one more, and about three coverages plus an odd remainder -- a thread's second and later grid-stride trips"""
    r = D.MODULUS[curve]
    w, ints, buf = pool(gpu, curve)
    a, b = buf.ptr.value, buf.ptr.value + 96 * 7                  # two overlapping windows of the pool: b[i] = pool[i + 7]
    for n in SIZES:
        assert as_int(curve, gpu.vec_dot(curve, a, b, n)) == H.dot(ints[:n], ints[7:7 + n], r), n
    for n in (CAP * 256 - 1, CAP * 256, CAP * 256 + 1, 3 * CAP * 256 + 77):
        want = H.dot(ints[:n], ints[7:7 + n], r)
        assert as_int(curve, capped(gpu, curve, 0, a, b, n, None, CAP)) == want, n
        assert as_int(curve, capped(gpu, curve, 0, a, b, n, None, 1)) == want, n
        assert as_int(curve, gpu.vec_dot(curve, a, b, n)) == want, n
    n = 3 * CAP * 256 + 77
    assert as_int(curve, gpu.vec_dot(curve, a, a, n)) == H.dot(ints[:n], ints[:n], r)          # dev_a == dev_b


@pytest.mark.parametrize("curve", [0, 1])
def test_vec_dot_edge_inputs(gpu, curve):
    """all r - 1 in both vectors (the operands the limb bounds are stated for), all zero, a single non-zero element at either end"""
    r = D.MODULUS[curve]
    n = 3 * CAP * 256 + 77
    top = dev(gpu, curve, [r - 1] * n)
    zero = dev(gpu, curve, [0] * n)
    for m in SIZES + [n]:
        assert as_int(curve, gpu.vec_dot(curve, top.ptr.value, top.ptr.value, m)) == m % r, m      # (-1)(-1) m
        assert not gpu.vec_dot(curve, zero.ptr.value, top.ptr.value, m).any()
    assert as_int(curve, capped(gpu, curve, 0, top.ptr.value, top.ptr.value, n, None, CAP)) == n % r
    w, ints, buf = pool(gpu, curve)
    for idx in (0, n - 1):
        one = [0] * n
        one[idx] = 5
        d1 = dev(gpu, curve, one)
        assert as_int(curve, gpu.vec_dot(curve, d1.ptr.value, buf.ptr.value, n)) == 5 * ints[idx] % r
        assert as_int(curve, capped(gpu, curve, 0, buf.ptr.value, d1.ptr.value, n, None, CAP)) == 5 * ints[idx] % r
        d1.close()
    top.close(); zero.close()


@pytest.mark.parametrize("curve", [0, 1])
def test_poly_eval(gpu, curve):
    """the sizes of the dot (a run is 16 coefficients, a block 4096) at t = 0, 1, r - 1 and a random t; under a cap of 2 blocks one
    coverage of the grid (8192 coefficients), one fewer, one more, and three coverages plus an odd remainder"""
    r = D.MODULUS[curve]
    w, ints, buf = pool(gpu, curve)
    c = buf.ptr.value
    cover = CAP * 256 * 16
    for t in (0, 1, r - 1, H.random_t(curve, 31)):
        t_w = H.wire1(curve, t)
        for n in SIZES + [15, 16, 17, 4095, 4096, 4097]:
            assert as_int(curve, gpu.poly_eval(curve, c, n, t_w)) == H.poly_eval(ints[:n], t, r), (t, n)
        for n in (cover - 1, cover, cover + 1, BIG):
            want = H.poly_eval(ints[:n], t, r)
            assert as_int(curve, capped(gpu, curve, 1, c, 0, n, t_w, CAP)) == want, (t, n)
            assert as_int(curve, gpu.poly_eval(curve, c, n, t_w)) == want, (t, n)
    t = H.random_t(curve, 32)
    for n in (1, 17, 4097, BIG):                                   # the only non-zero coefficient at n - 1
        last = [0] * n
        last[n - 1] = 3
        d1 = dev(gpu, curve, last)
        assert as_int(curve, gpu.poly_eval(curve, d1.ptr.value, n, H.wire1(curve, t))) == 3 * pow(t, n - 1, r) % r, n
        assert as_int(curve, capped(gpu, curve, 1, d1.ptr.value, 0, n, H.wire1(curve, t), CAP)) == 3 * pow(t, n - 1, r) % r, n
        d1.close()
    with pytest.raises(gpu.Mnt753Error):
        gpu.poly_eval(curve, c, 4, D.ints_to_words([r])[0])


DOMAINS = [(0, D.BASIC, 8), (0, D.BASIC, 1024), (0, D.STEP, 24), (0, D.STEP, 1024 + 8),
           (1, D.BASIC, 8), (1, D.BASIC, 1024), (1, D.STEP, 24), (1, D.STEP, 1024 + 8),
           (1, D.EXTENDED, 1 << 16), (1, D.MIXED, 40), (1, D.MIXED, 5 * 1024)]


def make_domain(gpu, curve, kind, m):
    if kind == D.BASIC:
        dom = gpu.Domain(curve, m)
    elif kind == D.MIXED:
        dom = gpu.Domain.mixed(curve, m)
    else:
        dom = gpu.Domain.for_size(curve, m)
    assert dom.m == m and dom.kind == Q.KIND_CODE[kind]
    return dom


def _did(p):
    return f"mnt{4 if p[0] == 0 else 6}-{p[1]}-{p[2]}"


@pytest.mark.parametrize("case", DOMAINS, ids=_did)
def test_interp_at(gpu, case):
    """k = 1 and 3 at a random t, t = 0 and t the last element of the domain (where the value is that element of each vector,
    exactly); dev_u receives the words of lagrange_at"""
    curve, kind, m = case
    r = D.MODULUS[curve]
    dom = make_domain(gpu, curve, kind, m)
    w, ints, buf = pool(gpu, curve)
    ptrs = [buf.ptr.value + 96 * off for off in (0, 11, 23)]       # three windows of the pool
    vecs = [ints[off:off + m] for off in (0, 11, 23)]
    u_buf = gpu.DeviceBuffer(96 * m)
    last = D.elements(curve, D.BASIC if kind == D.MIXED else kind, m)[-1]
    for t in (H.random_t(curve, 41), 0, last):
        t_w = H.wire1(curve, t)
        u = Q.lagrange_fast(curve, kind, m, t)
        want = [H.dot(v, u, r) for v in vecs]
        got3 = dom.interp_at(t_w, ptrs, u_ptr=u_buf.ptr.value)
        assert [as_int(curve, x) for x in got3] == want, t
        assert np.array_equal(u_buf.to_numpy().reshape(m, 12), dom.lagrange_at(t_w)), t
        got1 = dom.interp_at(t_w, ptrs[1:2])
        assert as_int(curve, got1[0]) == want[1], t
        if t == last:
            assert want == [v[m - 1] for v in vecs]
    u_buf.close(); dom.close()


def load_rows(directory):
    """ca, cb, cc (d + 1 rows each) of a fixture's input.bin"""
    d, m = (int(v) for v in np.fromfile(os.path.join(directory, "params.bin"), dtype=np.uint64, count=2))
    raw = np.fromfile(os.path.join(directory, "input.bin"), dtype=np.uint64).reshape(-1, 12)
    rest = raw[m + 1:]
    return d + 1, rest[:d + 1], rest[d + 1:2 * (d + 1)], rest[2 * (d + 1):3 * (d + 1)]


def accepted_cases():
    out = []
    for curve in (0, 1):
        out.append((f"g16-mnt{4 if curve == 0 else 6}", curve, None, os.path.dirname(fx(curve, "input.bin"))))
        out.append((f"cut21-mnt{4 if curve == 0 else 6}", curve, D.STEP, K.fixture_dir(curve, "cut21")))
    out.append(("extended-65536", 1, D.EXTENDED, 1 << 16))
    out.append(("mixed-5120", 1, D.MIXED, 5 * 1024))
    return out


def rows_of(gpu, curve, kind, src):
    """(domain, ca, cb, cc as wire arrays [m, 12]) with every row satisfied"""
    if isinstance(src, str):
        n, ca, cb, cc = load_rows(src)
        dom = gpu.Domain.for_size(curve, n)
        assert dom.m == n and (kind is None or dom.kind == Q.KIND_CODE[kind])
        return dom, ca, cb, cc
    m = src
    dom = make_domain(gpu, curve, kind, m)
    a = gpu.synth_scalars(curve, 0x61, m)
    b = gpu.synth_scalars(curve, 0x62, m)
    da, db = gpu.DeviceBuffer.from_numpy(a), gpu.DeviceBuffer.from_numpy(b)
    gpu.vec_muleq(curve, da.ptr.value, db.ptr.value, m)            # cc = ca cb by the element-wise product the transforms tests pin
    gpu.lib().mnt753_sync(None)
    c = da.to_numpy().reshape(m, 12)
    da.close(); db.close()
    return dom, a, b, c


KIND_OF_CODE = {v: k for k, v in Q.KIND_CODE.items()}


def model_sides(curve, dom, t, ca, cb, cc, h_w):
    """the model's (lhs, rhs) for wire arrays; L(t) in O(m)"""
    kind = KIND_OF_CODE[dom.kind]
    m = dom.m
    return H.sides(curve, kind, m, t, *(D.from_wire(curve, x) for x in (ca, cb, cc)), D.from_wire(curve, h_w))


def run_checked(gpu, dom, ca, cb, cc, t_w):
    bufs = [gpu.DeviceBuffer.from_numpy(x) for x in (ca, cb, cc)]
    dh = gpu.DeviceBuffer.from_numpy(np.full(12 * (dom.m + 1), PATTERN, dtype=np.uint64))
    try:
        res = dom.compute_h_checked(bufs[0].ptr.value, bufs[1].ptr.value, bufs[2].ptr.value, dh.ptr.value, t=t_w)
        return res, dh.to_numpy().reshape(dom.m + 1, 12)
    finally:
        for b in bufs + [dh]:
            b.close()


def plain_h(gpu, dom, ca, cb, cc):
    bufs = [gpu.DeviceBuffer.from_numpy(x) for x in (ca, cb, cc)]
    dh = gpu.DeviceBuffer(96 * (dom.m + 1))
    dom.compute_h(bufs[0].ptr.value, bufs[1].ptr.value, bufs[2].ptr.value, dh.ptr.value)
    gpu.lib().mnt753_sync(None)
    h = dh.to_numpy().reshape(dom.m + 1, 12)
    for b in bufs:
        b.close()
    return h, dh


@pytest.mark.parametrize("case", accepted_cases(), ids=lambda c: c[0])
def test_compute_h_checked_accepts(gpu, case):
    """satisfied rows: ok, h word for word the h of compute_h, lhs and rhs the model's; then the three-call form (interp_at before
    compute_h, h_check after) gives the same"""
    _, curve, kind, src = case
    dom, ca, cb, cc = rows_of(gpu, curve, kind, src)
    t = H.random_t(curve, 51)
    t_w = H.wire1(curve, t)
    h, dh = plain_h(gpu, dom, ca, cb, cc)
    (ok, lhs, rhs), h2 = run_checked(gpu, dom, ca, cb, cc, t_w)
    assert np.array_equal(h, h2)
    want = model_sides(curve, dom, t, ca, cb, cc, h)
    assert want[0] == want[1] and want[0] != 0
    assert ok and (as_int(curve, lhs), as_int(curve, rhs)) == want
    bufs = [gpu.DeviceBuffer.from_numpy(x) for x in (ca, cb, cc)]
    abc = dom.interp_at(t_w, [b.ptr.value for b in bufs])
    ok3, lhs3, rhs3 = dom.h_check(t_w, abc, dh.ptr.value)
    assert ok3 and np.array_equal(lhs3, lhs) and np.array_equal(rhs3, rhs)
    (ok_r, _, _), _ = run_checked(gpu, dom, ca, cb, cc, None)       # t from the operating system: a satisfied system passes at any t
    assert ok_r
    for b in bufs + [dh]:
        b.close()
    dom.close()


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("logm", [3, 8])
def test_check_rejects_the_reference_h_of_unsatisfied_rows(gpu, curve, logm):
    """tests/golden/h_mnt{4,6}_{3,8}.bin: random ca / cb / cc whose rows are not satisfied, and the reference's own h for them"""
    ca, cb, cc, h_ref = G.h(curve, logm)
    dom = gpu.Domain(curve, 1 << logm)
    t = H.random_t(curve, 61 + logm)
    (ok, lhs, rhs), h = run_checked(gpu, dom, ca, cb, cc, H.wire1(curve, t))
    assert np.array_equal(h, h_ref)
    want = model_sides(curve, dom, t, ca, cb, cc, h_ref)
    assert want[0] != want[1]
    assert not ok and (as_int(curve, lhs), as_int(curve, rhs)) == want
    dom.close()


@pytest.mark.parametrize("case", [c for c in accepted_cases() if c[0] in ("cut21-mnt4", "g16-mnt6", "mixed-5120")], ids=lambda c: c[0])
def test_check_rejects_one_changed_value(gpu, case):
    """one cc changed before compute_h; one coefficient of a clean h changed on the device -- at 0, m - 2, m - 1, m (the appended
    zero) and at the edges of a run (15 | 16) and of a block (4095 | 4096) of k_poly_eval where the domain reaches them; two
    coefficients swapped.  The model predicts every verdict and both sides."""
    _, curve, kind, src = case
    r = D.MODULUS[curve]
    dom, ca, cb, cc = rows_of(gpu, curve, kind, src)
    m = dom.m
    t = H.random_t(curve, 71)
    t_w = H.wire1(curve, t)
    cc2 = cc.copy()
    cc2[m // 3] = H.wire1(curve, (as_int(curve, cc[m // 3]) + 1) % r)
    (ok, lhs, rhs), h_bad = run_checked(gpu, dom, ca, cb, cc2, t_w)
    want = model_sides(curve, dom, t, ca, cb, cc2, h_bad)
    assert want[0] != want[1] and not ok and (as_int(curve, lhs), as_int(curve, rhs)) == want
    h, dh = plain_h(gpu, dom, ca, cb, cc)
    bufs = [gpu.DeviceBuffer.from_numpy(x) for x in (ca, cb, cc)]
    abc = dom.interp_at(t_w, [b.ptr.value for b in bufs])
    assert dom.h_check(t_w, abc, dh.ptr.value)[0]
    h_int = D.from_wire(curve, h)
    a_t, b_t, c_t = (as_int(curve, x) for x in abc)
    z = Q.vanishing(curve, KIND_OF_CODE[dom.kind], m, t)
    for idx in sorted({0, m - 2, m - 1, m} | {i for i in (15, 16, 4095, 4096) if i < m}):
        h2 = list(h_int)
        h2[idx] = (h2[idx] + 1) % r
        gpu.lib().mnt753_copy_h2d(ctypes.c_void_p(dh.ptr.value + 96 * idx), ctypes.c_void_p(H.wire1(curve, h2[idx]).ctypes.data), 96)
        ok, lhs, rhs = dom.h_check(t_w, abc, dh.ptr.value)
        assert not ok and as_int(curve, rhs) == z * H.poly_eval(h2, t, r) % r and as_int(curve, lhs) == (a_t * b_t - c_t) % r, idx
        gpu.lib().mnt753_copy_h2d(ctypes.c_void_p(dh.ptr.value + 96 * idx), ctypes.c_void_p(np.ascontiguousarray(h[idx]).ctypes.data), 96)
    assert dom.h_check(t_w, abc, dh.ptr.value)[0]                   # restored
    i, j = 1, m - 3
    assert h_int[i] != h_int[j]
    for dst, src_row in ((i, h[j]), (j, h[i])):
        gpu.lib().mnt753_copy_h2d(ctypes.c_void_p(dh.ptr.value + 96 * dst), ctypes.c_void_p(np.ascontiguousarray(src_row).ctypes.data), 96)
    assert not dom.h_check(t_w, abc, dh.ptr.value)[0]
    for b in bufs + [dh]:
        b.close()
    dom.close()


@pytest.mark.parametrize("curve,kind,m", [(0, D.BASIC, 8), (1, D.STEP, 24), (1, D.MIXED, 40)])
def test_check_refuses_t_inside_the_domain_and_t_above_r(gpu, curve, kind, m):
    """Z(t) = 0 would say nothing about H; t >= r is no element: MNT753_EINVAL, and the vectors, h and the result stay as they were"""
    r = D.MODULUS[curve]
    dom = make_domain(gpu, curve, kind, m)
    ca, cb, cc = H.satisfied_rows(curve, m, 81)
    rows = [D.to_wire(curve, v) for v in (ca, cb, cc)]
    inside = [H.wire1(curve, x) for x in (D.elements(curve, D.BASIC if kind == D.MIXED else kind, m)[i] for i in (0, m // 2, m - 1))]
    bad = inside + [D.ints_to_words([r])[0], np.full(12, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)]
    bufs = [gpu.DeviceBuffer.from_numpy(x) for x in rows]
    fill = np.full(12 * (m + 1), PATTERN, dtype=np.uint64)
    dh = gpu.DeviceBuffer.from_numpy(fill)
    L = gpu.lib()
    u64p = ctypes.POINTER(ctypes.c_uint64)
    for t_w in bad:
        t_w = np.ascontiguousarray(t_w, dtype=np.uint64)
        res = gpu.HCheckResult()
        res.ok, res.reserved = 7, 9
        rc = L.mnt753_compute_h_checked(dom._h, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, dh.ptr, t_w.ctypes.data_as(u64p), ctypes.byref(res), None)
        assert rc == -1
        abc = np.zeros(36, dtype=np.uint64)
        rc = L.mnt753_h_check(dom._h, t_w.ctypes.data_as(u64p), abc.ctypes.data_as(u64p), dh.ptr, ctypes.byref(res), None)
        assert rc == -1
        assert (res.ok, res.reserved) == (7, 9) and not any(res.lhs) and not any(res.rhs)
    L.mnt753_sync(None)
    assert np.array_equal(dh.to_numpy(), fill)
    for b, x in zip(bufs, rows):
        assert np.array_equal(b.to_numpy().reshape(m, 12), x)
    for b in bufs + [dh]:
        b.close()
    dom.close()


# ---- main_hip --check-h -----------------------------------------------------------------------------------------------------------------
MESSAGE = "H: H·Z = A·B − C fails at t = 0x"


def t_file(tmp_path, curve):
    t_w = H.wire1(curve, H.random_t(curve, 91))
    path = tmp_path / "t.bin"
    t_w.tofile(path)
    return str(path), t_w


def broken_input(tmp_path, curve):
    """a copy of the e2e input with the lowest bit of one cc word flipped: one row no longer has ca cb = cc"""
    params, inp, _ = G.e2e_paths(curve)
    d, m = (int(v) for v in np.fromfile(params, dtype=np.uint64, count=2))
    raw = bytearray(open(inp, "rb").read())
    assert len(raw) == 96 * ((m + 1) + 3 * (d + 1) + 1)
    raw[96 * ((m + 1) + 2 * (d + 1) + (d + 1) // 2)] ^= 1
    path = tmp_path / "input_bad.bin"
    path.write_bytes(raw)
    return str(path)


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("flags,env", [([], {}), (["--unfused-h"], {}), (["--gpus", "3"], {"MNT753_SHARE_DEVICE": "1"}),
                                       (["--gpus", "3", "--unfused-h", "--ref-order"], {"MNT753_SHARE_DEVICE": "1"})],
                         ids=["fused", "unfused", "sharded", "sharded-unfused"])
def test_cli_check_h_keeps_the_proof_bytes(gpu, curve, flags, env, tmp_path):
    params, inp, expected = G.e2e_paths(curve)
    tf, _ = t_file(tmp_path, curve)
    out = tmp_path / "proof.bin"
    r = subprocess.run([EXE, NAME[curve], "compute", params, inp, str(out), "--check-h", "--check-h-t", tf] + flags, capture_output=True, text=True,
                       env=dict(os.environ, **env))
    assert r.returncode == 0, r.stderr
    assert "check H: H Z = A B - C holds" in r.stdout
    assert out.read_bytes() == open(expected, "rb").read()


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("flags,env", [([], {}), (["--unfused-h"], {}), (["--gpus", "3"], {"MNT753_SHARE_DEVICE": "1"})], ids=["fused", "unfused", "sharded"])
def test_cli_check_h_refuses_a_broken_row(gpu, curve, flags, env, tmp_path):
    """without --validate: the row check is not run, the identity catches the row.  Exit 3, no output file, the message with t."""
    params, _, _ = G.e2e_paths(curve)
    bad = broken_input(tmp_path, curve)
    tf, t_w = t_file(tmp_path, curve)
    out = tmp_path / "proof.bin"
    r = subprocess.run([EXE, NAME[curve], "compute", params, bad, str(out), "--check-h-t", tf] + flags, capture_output=True, text=True,
                       env=dict(os.environ, **env))
    assert r.returncode == 3, r.stderr
    assert not out.exists()
    t_hex = "%x" % int.from_bytes(t_w.tobytes(), "little")
    assert MESSAGE + t_hex in r.stderr, r.stderr
    # the same input without the check is proved as before (nothing else looks at the rows)
    r = subprocess.run([EXE, NAME[curve], "compute", params, bad, str(out)] + flags, capture_output=True, text=True, env=dict(os.environ, **env))
    assert r.returncode == 0 and out.exists()


def test_cli_check_h_goes_on_with_the_next_job(gpu, tmp_path):
    """two jobs in one process, the first one bad: the second proof is written, the process exits 3; a random t per job (MNT753_CHECK_H)"""
    curve = 0
    params, inp, expected = G.e2e_paths(curve)
    bad = broken_input(tmp_path, curve)
    o1, o2 = tmp_path / "p1.bin", tmp_path / "p2.bin"
    env = dict(os.environ, MNT753_CHECK_H="1")
    r = subprocess.run([EXE, NAME[curve], "compute", params, bad, str(o1), inp, str(o2)], capture_output=True, text=True, env=env)
    assert r.returncode == 3, r.stderr
    assert not o1.exists() and o2.read_bytes() == open(expected, "rb").read()
    assert MESSAGE in r.stderr and f"failed {o1}" in r.stdout


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("env", [{}, {"MNT753_GPUS": "3", "MNT753_SHARE_DEVICE": "1"}], ids=["one-device", "sharded"])
def test_wrapper_check_h_inside_compute_h_fused(gpu, curve, env, tmp_path):
    """B::check_H(true): B::compute_H_fused takes A(t), B(t), C(t) before its transforms (sharded: each vector where it lives) and
    throws h_check_failed behind them where the identity fails (tools/host_tests/h_check_wrapper_test.cpp)"""
    exe = os.path.join(os.path.dirname(EXE), "h_check_wrapper_test")
    params, inp, _ = G.e2e_paths(curve)
    r = subprocess.run([exe, NAME[curve], params, inp], capture_output=True, text=True, env=dict(os.environ, **env))
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
    r = subprocess.run([exe, NAME[curve], params, broken_input(tmp_path, curve)], capture_output=True, text=True, env=dict(os.environ, **env))
    assert r.returncode == 3 and r.stdout.startswith("refused: " + MESSAGE), r.stdout + r.stderr
