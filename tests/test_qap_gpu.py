"""GPU: the QAP at a point (mnt753_domain_lagrange_at / _vanishing_at, mnt753_vec_powers, mnt753_r1cs_qap_at, `main_hip qap-at`)
against the reference-minted fixture tests/golden/qap (tools/mint_qap.sh) and the Python model tests/qap_ref.py, which
tests/test_qap_cpu.py pins to that fixture.  Every value is an exact field element: equal means equal words."""
import os
import subprocess

import numpy as np
import pytest

import domain_ref as D
import qap_ref as Q
from test_groth16_cpu import EXE, NAME, fx, load_input

pytestmark = pytest.mark.gpu

INDEX = Q.index()
PATTERN = 0xA5A5A5A5A5A5A5A5


def _id(e):
    return f"mnt{4 if e['curve'] == 0 else 6}-{e['kind']}-{e['m']}"


def make_domain(gpu, entry):
    curve, kind, m = entry["curve"], entry["kind"], entry["m"]
    if kind == D.BASIC:
        dom = gpu.Domain(curve, m)
    elif kind == D.MIXED:
        dom = gpu.Domain.mixed(curve, m)
    else:
        dom = gpu.Domain.for_size(curve, m)
    assert dom.m == m and dom.kind == Q.KIND_CODE[kind]
    return dom


@pytest.mark.parametrize("entry", INDEX["lagrange"], ids=_id)
def test_lagrange_and_vanishing_equal_the_reference(gpu, entry):
    """every record of the fixture: the generic t, t = 0, and t = a domain element of either half (the indicator vectors).  In full
    below 2^16; the 2^16 extended domain by sha256 and on the sample.  Sub-domains shorter than one inversion run (2, 8, 16 + 8) and
    domains over several workgroups (1024, 1152, 2^16) are among the sizes."""
    dom = make_domain(gpu, entry)
    for label, t_w, zt_w, u_w, idx, sha in Q.lagrange_records(entry):
        assert dom.vanishing_at(t_w).tolist() == zt_w.tolist(), label
        u = dom.lagrange_at(t_w)
        assert Q.sha256_words(u) == sha, label
        assert np.array_equal(u if idx is None else u[idx], u_w), label
    dom.close()


@pytest.mark.parametrize("curve", [0, 1])
def test_vec_powers(gpu, curve):
    """1, t, .., t^(n-1) for lengths around the run of one thread and over more than one block"""
    t_w = gpu.synth_scalars(curve, 0x51, 1)[0]
    t, r = D.from_wire(curve, t_w)[0], D.MODULUS[curve]
    want, x = [], 1
    for _ in range(4133):
        want.append(x)
        x = x * t % r
    want = D.to_wire(curve, want)
    for n in (1, 15, 16, 17, 4133):
        assert np.array_equal(gpu.vec_powers(curve, t_w, n), want[:n]), n
    assert gpu.vec_powers(curve, t_w, 0).shape[0] == 0
    zero = np.zeros(12, dtype=np.uint64)
    assert np.array_equal(gpu.vec_powers(curve, zero, 3), D.to_wire(curve, [1, 0, 0]))


def run_qap_at(gpu, cs, dom, t_w):
    at, bt, ct, ht, zt = cs.qap_at(dom, t_w)
    gpu.lib().mnt753_sync(None)
    out = [b.to_numpy().reshape(-1, 12) for b in (at, bt, ct, ht)]
    for b in (at, bt, ct, ht):
        b.close()
    return out + [zt]


@pytest.mark.parametrize("entry", INDEX["qap"], ids=lambda e: f"mnt{4 if e['curve'] == 0 else 6}")
def test_qap_at_equals_the_reference(gpu, entry):
    """At, Bt, Ct, Ht, Zt of r1cs_to_qap_instance_map_with_evaluation on the g16 fixture's constraint system"""
    curve = entry["curve"]
    cs = gpu.R1cs.from_file(curve, fx(curve, "r1cs.bin"))
    dom = gpu.Domain.for_size(curve, cs.domain_size())
    assert dom.m == entry["m"]
    t_w, *want = Q.qap_record(entry)
    got = run_qap_at(gpu, cs, dom, t_w)
    for g, w in zip(got, want):
        assert np.array_equal(g.reshape(w.shape), w)
    plan = cs.qap_plan()
    assert plan["terms"] == sum(int(m[0][-1]) for m in gpu.read_r1cs_file(fx(curve, "r1cs.bin"))[3]) and plan["chunk_terms"] >= 1
    cs.close(); dom.close()


def test_qap_at_on_two_streams(gpu):
    """two calls on one system on different streams share its copy of u and its partial sums: the second is ordered behind the first
    on the device, and both give the reference's words (different points, so a mixed-up u would show)"""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")                    # the runtime the library is linked against: two streams of its own
    streams = [C.c_void_p(), C.c_void_p()]
    for st in streams:
        assert hip.hipStreamCreate(C.byref(st)) == 0
    entry = INDEX["qap"][0]
    curve = entry["curve"]
    cs = gpu.R1cs.from_file(curve, fx(curve, "r1cs.bin"))
    dom = gpu.Domain.for_size(curve, cs.domain_size())
    t_w, *want = Q.qap_record(entry)
    t2_w = gpu.synth_scalars(curve, 0x53, 1)[0]
    r1 = cs.qap_at(dom, t_w, stream=streams[0].value)
    r2 = cs.qap_at(dom, t2_w, stream=streams[1].value)
    r3 = cs.qap_at(dom, t_w, stream=streams[0].value)
    for st in streams:
        assert gpu.lib().mnt753_sync(st) == 0
    for res in (r1, r3):
        for b, w in zip(res[:4], want[:4]):
            assert np.array_equal(b.to_numpy().reshape(w.shape), w)
        assert res[4].tolist() == want[4].tolist()
    t2 = D.from_wire(curve, t2_w)[0]
    ht2 = D.to_wire(curve, [pow(t2, i, D.MODULUS[curve]) for i in range(dom.m + 1)])
    assert np.array_equal(r2[3].to_numpy().reshape(-1, 12), ht2)
    assert not np.array_equal(r2[0].to_numpy(), r1[0].to_numpy())
    for res in (r1, r2, r3):
        for b in res[:4]:
            b.close()
    cs.close(); dom.close()
    for st in streams:
        assert hip.hipStreamDestroy(st) == 0


def designed_system(gpu, curve, nc, m, L):
    """The ragged system of test_device_witness_evaluation_vs_oracle_random_system (rows of 0 .. 9 terms) with designed columns:
    column 0 holds 4 L + 3 terms, columns 7, 8, 9, 10 exactly L - 1, L, L + 1, 2 L + 1, column 12 none; some (row, col) pairs repeat;
    every 17th coefficient is zero."""
    rng = np.random.default_rng(70 + curve)
    special = (4 * L + 3, L - 1, L, L + 1, 2 * L + 1)
    special_cols = (0, 7, 8, 9, 10)
    mats = []
    for k in range(3):
        counts = rng.integers(0, 10, size=nc); counts[0] = 0
        rp = np.zeros(nc + 1, dtype=np.uint64); rp[1:] = np.cumsum(counts)
        nnz = int(rp[nc])
        col = rng.integers(0, m + 1, size=nnz).astype(np.uint32)
        col[np.isin(col, special_cols + (12,))] = 13
        order, pos = rng.permutation(nnz), 0
        for c, n in zip(special_cols, special):
            col[order[pos:pos + n]] = c
            pos += n
        dup = 0
        for row in range(1, nc):                      # repeat a (row, col) pair in rows whose first two terms are free
            a = int(rp[row])
            if counts[row] >= 2 and col[a] > 13 and col[a + 1] > 13:
                col[a + 1] = col[a]
                dup += 1
                if dup == 40:
                    break
        assert dup == 40
        cf = gpu.synth_scalars(curve, 140 + k, nnz)
        cf[::17] = 0
        for c, n in zip(special_cols, special):
            assert int((col == c).sum()) == n
        assert not (col == 12).any()
        mats.append((rp, col, cf))
    return mats


@pytest.mark.parametrize("curve", [0, 1])
def test_qap_at_on_designed_columns(gpu, curve):
    """against the model: columns of more than 4 L, of L - 1, L, L + 1 and 2 L + 1 terms, an empty column in each matrix, repeated
    (row, col) pairs, zero coefficients.  MNT4753: the 8192-point basic domain; MNT6753: the mixed domain of 5 * 2^10 elements."""
    m, num_inputs = 3000, 3
    nc = 5000 if curve == 0 else 5116
    probe = gpu.R1cs.from_file(curve, fx(curve, "r1cs.bin"))
    L = probe.qap_plan()["chunk_terms"]
    probe.close()
    mats = designed_system(gpu, curve, nc, m, L)
    cs = gpu.R1cs(curve, num_inputs, m, nc, mats)
    if curve == 0:
        dom, kind = gpu.Domain(curve, 8192), D.BASIC
    else:
        dom, kind = gpu.Domain.for_size(curve, nc + num_inputs + 1, mixed=True), D.MIXED
        assert dom.m == 5 * 1024 and dom.kind == gpu.Domain.MIXED
    plan = cs.qap_plan()
    assert plan["chunk_terms"] == L and plan["longest_column"] == 4 * L + 3
    assert plan["split_columns"] == 9                 # per matrix: 4 L + 3, L + 1 and 2 L + 1 terms
    assert plan["terms"] == sum(int(rp[nc]) for rp, _, _ in mats) and plan["work_items"] > 3 * 8
    t_w = gpu.synth_scalars(curve, 0x52, 1)[0]
    t = D.from_wire(curve, t_w)[0]
    u = Q.lagrange_fast(curve, kind, dom.m, t)
    imats = [(rp, col, D.from_wire(curve, cf)) for rp, col, cf in mats]
    want = Q.instance_map(curve, num_inputs, nc, m, imats, u, t, dom.m)
    got = run_qap_at(gpu, cs, dom, t_w)
    for g, w in zip(got, want):
        assert np.array_equal(g, D.to_wire(curve, w))
    assert got[4].tolist() == D.to_wire(curve, [Q.vanishing(curve, kind, dom.m, t)])[0].tolist()
    for k in (1, 2):
        assert not got[k][12].any()                   # the empty column is written as zero
    again = run_qap_at(gpu, cs, dom, t_w)             # a second call on the kept view gives the same words
    for g, a in zip(got, again):
        assert np.array_equal(g, a)
    cs.close(); dom.close()


@pytest.mark.parametrize("curve", [0, 1])
def test_qap_identity_with_compute_h(gpu, curve):
    """(sum w_i At_i)(sum w_i Bt_i) - sum w_i Ct_i = Zt sum h_i Ht_i (mod r) with h from the device compute_h on the fixture's
    ca / cb / cc: ties the evaluation to the compute_H that is pinned to the reference; violated once a witness element changes."""
    d, m, w_w, ca, cb, cc, _ = load_input(curve)
    r = D.MODULUS[curve]
    dom = gpu.Domain.for_size(curve, d + 1)
    bufs = [gpu.DeviceBuffer.from_numpy(x) for x in (ca, cb, cc)]
    dh = gpu.DeviceBuffer(96 * (d + 2))
    dom.compute_h(bufs[0].ptr.value, bufs[1].ptr.value, bufs[2].ptr.value, dh.ptr.value)
    h = D.from_wire(curve, dh.to_numpy().reshape(d + 2, 12))
    cs = gpu.R1cs.from_file(curve, fx(curve, "r1cs.bin"))
    t_w = np.fromfile(os.path.join(Q.GOLDEN, f"t_mnt{4 if curve == 0 else 6}.bin"), dtype=np.uint64)
    at, bt, ct, ht, zt = (D.from_wire(curve, x) for x in run_qap_at(gpu, cs, dom, t_w))
    w = D.from_wire(curve, w_w)
    assert len(at) == len(w) == m + 1 and len(ht) == len(h) == d + 2
    dot = lambda a, b: sum(x * y for x, y in zip(a, b)) % r
    rhs = zt[0] * dot(h, ht) % r
    assert (dot(w, at) * dot(w, bt) - dot(w, ct)) % r == rhs
    assert any(h) and any(at) and zt[0] != 0
    w2 = list(w); w2[2] = (w2[2] + 1) % r
    assert (dot(w2, at) * dot(w2, bt) - dot(w2, ct)) % r != rhs
    cs.close(); dom.close()


def test_refusals_leave_the_outputs_untouched(gpu):
    """a domain of the other curve, a domain smaller than the system, t >= r: Mnt753Error, and nothing is written"""
    curve = 0
    cs = gpu.R1cs.from_file(curve, fx(curve, "r1cs.bin"))
    nv, need = cs.m + 1, cs.domain_size()
    good, other, small = gpu.Domain(curve, 32), gpu.Domain(1, 32), gpu.Domain(curve, 16)
    assert need == 32
    t_w = gpu.synth_scalars(curve, 0x51, 1)[0]
    big_t = np.full(12, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)                      # >= r
    r_w = D.ints_to_words([D.MODULUS[curve]])[0]                                  # r itself
    fill = np.full(12 * (3 * nv + 33), PATTERN, dtype=np.uint64)
    buf = gpu.DeviceBuffer.from_numpy(fill)
    p = buf.ptr.value
    out = (p, p + 96 * nv, p + 192 * nv, p + 288 * nv)
    for dom, t in ((other, t_w), (small, t_w), (good, big_t), (good, r_w)):
        with pytest.raises(gpu.Mnt753Error):
            cs.qap_at(dom, t, out=out)
    for t in (big_t, r_w):
        with pytest.raises(gpu.Mnt753Error):
            good.lagrange_at(t, out_ptr=p)
        with pytest.raises(gpu.Mnt753Error):
            good.vanishing_at(t)
        with pytest.raises(gpu.Mnt753Error):
            gpu.vec_powers(curve, t, 4, out_ptr=p)
    gpu.lib().mnt753_sync(None)
    assert np.array_equal(buf.to_numpy(), fill)
    cs.qap_at(good, t_w, out=out)                                                 # the same buffers are written by a good call
    gpu.lib().mnt753_sync(None)
    assert not (buf.to_numpy() == PATTERN).any()
    for x in (cs, good, other, small, buf):
        x.close()


@pytest.mark.parametrize("curve", [0, 1])
def test_main_hip_qap_at(gpu, curve, tmp_path):
    """main_hip <curve> qap-at <r1cs> <t_file> <output> writes At | Bt | Ct | Ht | Zt of the fixture; a t file of 95 bytes or with a
    value >= r exits 1 and writes nothing"""
    name = f"mnt{4 if curve == 0 else 6}"
    t_file, want = os.path.join(Q.GOLDEN, f"t_{name}.bin"), open(os.path.join(Q.GOLDEN, f"qap_{name}.bin"), "rb").read()
    out = tmp_path / "qap.bin"
    r = subprocess.run([EXE, NAME[curve], "qap-at", fx(curve, "r1cs.bin"), t_file, str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == want
    short, over, none = tmp_path / "short.bin", tmp_path / "over.bin", tmp_path / "none.bin"
    short.write_bytes(open(t_file, "rb").read()[:95])
    over.write_bytes(b"\xff" * 96)
    for bad in (short, over):
        r = subprocess.run([EXE, NAME[curve], "qap-at", fx(curve, "r1cs.bin"), str(bad), str(none)], capture_output=True, text=True)
        assert r.returncode == 1 and r.stderr.strip() and not none.exists(), r.stderr
    r = subprocess.run([EXE, NAME[curve], "qap-at", fx(curve, "r1cs.bin"), t_file], capture_output=True, text=True)
    assert r.returncode == 2 and "qap-at" in r.stderr
