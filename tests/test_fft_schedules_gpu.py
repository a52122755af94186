"""GPU: the radix-2 NTT at EVERY pass schedule and on structured inputs, bit-exact against the oracle and against closed forms.

run_stages splits the log2 m stages of a transform into ceil(log2 m / 8) launches of k_ntt_group of balanced width
(fft_structured.schedule).  The cases here, by log2 m and group widths (the test ids carry them):

    1 ... 8      one group of that width                       17 ... 24    6+6+5, 6+6+6, 7+6+6, 7+7+6, 7+7+7, 8+7+7, 8+8+7, 8+8+8
    9 ... 16     5+4, 5+5, 6+5, 6+6, 7+6, 7+7, 8+7, 8+8        25           7+6+6+6: the first four-group schedule

so every width 1 ... 8 is a first group, 4 ... 8 a last group behind another one, and the inner groups (no bit reversal, no scale)
take widths 6, 7 and 8.  MNT4753 runs all of them, MNT6753 those up to 2^15 (its Fr has two-adicity 15).

Uniform random data sits mid-range in the carry-free butterflies and never gives an output that is 0 mod r; the kernels
normalise only every second stage, so such an output reaches fp_canon as the lazy representative p.  The structured vectors of
tests/fft_structured.py (mostly-zero transforms, operands pinned at the word pattern r - 1) go through whole kernels here, and
likewise through the folds of the step / extended passes, the two-terms-per-normalisation accumulation of k_r1cs_evaluate and the
element-wise vector kernels (with both operands the same pointer).  Every comparison is of whole vectors, word for word."""
import time

import numpy as np
import pytest

import domain_ref as D
import fft_structured as S
import oracle_lib as O

pytestmark = pytest.mark.gpu

NAME = {0: "mnt4", 1: "mnt6"}
SWEEP = [(0, logm) for logm in range(1, 21)] + [(1, logm) for logm in range(1, 16)]


def case_id(curve, logm):
    return f"{NAME[curve]}-2^{logm}-" + "+".join(str(ns) for ns in S.schedule(logm))


SWEEP_PARAMS = [pytest.param(c, l, id=case_id(c, l)) for c, l in SWEEP]


def on_gpu(gpu, vec, fn):
    """fn(device pointer) on a device copy of the wire array vec -> the array afterwards"""
    buf = gpu.DeviceBuffer.from_numpy(np.ascontiguousarray(vec, dtype=np.uint64))
    try:
        fn(buf.ptr.value)
        return buf.to_numpy().reshape(-1, 12)
    finally:
        buf.close()


def planted(gpu, curve, seed, m):
    """synth_scalars with 0, the Montgomery one and r - 1 at indices 0, 1, m/2 and m - 1 (where they exist; the later index wins)"""
    v = gpu.synth_scalars(curve, seed, m)
    edge = S.words([0, S.mont_one(curve), S.modulus(curve) - 1])
    for idx, e in ((0, 0), (1, 1), (m // 2, 2), (m - 1, 2)):
        if idx < m:
            v[idx] = edge[e]
    return v


# ---- B: every schedule against the oracle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve,logm", SWEEP_PARAMS)
@pytest.mark.timeout(600)
def test_every_schedule_four_kinds_and_divide_by_z(gpu, curve, logm):
    m = 1 << logm
    v = planted(gpu, curve, 2000 + logm, m)
    dom = gpu.Domain(curve, m)
    try:
        for kind in S.KINDS:
            got = on_gpu(gpu, v, lambda p: dom.fft(kind, p))
            assert np.array_equal(got, O.fft(curve, kind, v).reshape(m, 12)), f"kind {kind}"
        got = on_gpu(gpu, v, dom.divide_by_z_on_coset)
        assert np.array_equal(got, O.divide_by_z_on_coset(curve, v).reshape(m, 12)), "divide_by_Z_on_coset"
    finally:
        dom.close()


def compute_h_three_ways(gpu, dom, curve, ca, cb, cc):
    """compute_h; compute_h_chain x3 + compute_h_finish; the unfused sequence of B:: calls (cuda_prover_piecewise.cu:24-47)
    -> three [m + 1, 12] arrays (the last one with its zero row appended here)"""
    m = ca.shape[0]
    outs = []
    for split in (False, True):
        a, b, c = (gpu.DeviceBuffer.from_numpy(x) for x in (ca, cb, cc))
        dh = gpu.DeviceBuffer(96 * (m + 1))
        try:
            if split:
                for x in (a, b, c):
                    dom.compute_h_chain(x.ptr.value)
                dom.compute_h_finish(a.ptr.value, b.ptr.value, c.ptr.value, dh.ptr.value)
            else:
                dom.compute_h(a.ptr.value, b.ptr.value, c.ptr.value, dh.ptr.value)
            outs.append(dh.to_numpy().reshape(m + 1, 12))
        finally:
            for x in (a, b, c, dh):
                x.close()
    a, b, c = (gpu.DeviceBuffer.from_numpy(x) for x in (ca, cb, cc))
    try:
        for x in (a, b):
            dom.fft(gpu.IFFT, x.ptr.value)
        for x in (a, b):
            dom.fft(gpu.COSET_FFT, x.ptr.value)
        gpu.vec_muleq(curve, a.ptr.value, b.ptr.value, m)
        dom.fft(gpu.IFFT, c.ptr.value); dom.fft(gpu.COSET_FFT, c.ptr.value)
        gpu.vec_subeq(curve, a.ptr.value, c.ptr.value, m)
        dom.divide_by_z_on_coset(a.ptr.value)
        dom.fft(gpu.ICOSET_FFT, a.ptr.value)
        outs.append(np.concatenate([a.to_numpy().reshape(m, 12), np.zeros((1, 12), dtype=np.uint64)]))
    finally:
        for x in (a, b, c):
            x.close()
    return outs


@pytest.mark.parametrize("curve,logm", SWEEP_PARAMS)
@pytest.mark.timeout(600)
def test_every_schedule_compute_h(gpu, curve, logm):
    m = 1 << logm
    ca, cb, cc = (planted(gpu, curve, 3000 + 3 * logm + k, m) for k in range(3))
    want = O.compute_h(curve, ca, cb, cc).reshape(m + 1, 12)
    dom = gpu.Domain(curve, m)
    try:
        for how, got in zip(("compute_h", "chain x3 + finish", "unfused"), compute_h_three_ways(gpu, dom, curve, ca, cb, cc)):
            assert np.array_equal(got, want), how
    finally:
        dom.close()


# 2^21 ... 2^25 on MNT4753: seconds per case measured on an MI355X host (the oracle's OpenMP butterfly loops on 16 threads take
# 2.6, 5.3, 11.2, 22.6 and 43.2 s of them); the timeout of each case is three times its measurement.
LARGE_SECONDS = {21: 3.3, 22: 6.5, 23: 13.9, 24: 27.9, 25: 53.4}
LARGE_N = 1 << 10


@pytest.mark.parametrize("logm", [pytest.param(l, id=case_id(0, l), marks=pytest.mark.timeout(int(3 * LARGE_SECONDS[l]) + 1))
                                  for l in sorted(LARGE_SECONDS)])
def test_large_schedules(gpu, logm):
    """Three- and four-group schedules above every size the rest of the suite runs (7+7+7, 8+7+7, 8+8+7, 8+8+8, 7+6+6+6).
    cosetFFT of a planted seeded vector, whole vector against the oracle (<IN_SCALE> on the first group, the plain instantiation on
    the inner ones); icosetFFT of that result gives the input words back (with the forward result pinned this pins tw_inv, cos_inv_s
    and <OUT_SCALE> at the size); the period-2^10 and the zero-stuffed vector through FFT and iFFT with every one of the m outputs
    checked against the closed form.  One domain (544 B per element) and one device vector (96 B per element) at a time.
    Measured: 3.3, 6.5, 13.9, 27.9 and 53.4 s for 2^21 ... 2^25 (LARGE_SECONDS); the whole file takes 200 s."""
    m = 1 << logm
    t0 = time.time()
    v = planted(gpu, 0, 4000 + logm, m)
    dom = gpu.Domain(0, m)
    d = None
    try:
        d = gpu.DeviceBuffer.from_numpy(v)
        dom.fft(gpu.COSET_FFT, d.ptr.value)
        got = d.to_numpy().reshape(m, 12)
        t1 = time.time()
        want = O.fft(0, S.COSET_FFT, v).reshape(m, 12)
        t2 = time.time()
        assert np.array_equal(got, want), "cosetFFT against the oracle"
        del got, want
        dom.fft(gpu.ICOSET_FFT, d.ptr.value)
        assert np.array_equal(d.to_numpy().reshape(m, 12), v), "icosetFFT(cosetFFT(v)) != v"
        d.close(); d = None
        del v
        # period n and zero-stuffed, n = 2^10: the non-zero outputs / the repeated block come from a size-n transform in Python
        n, t = LARGE_N, m // LARGE_N
        seed = S.seeded(0, 4100 + logm, 2 * n)
        per, stu = seed[:n - 1] + [S.modulus(0) - 1], seed[n:]
        for kind in (S.FFT, S.IFFT):
            vec = np.tile(S.words(per), (t, 1))
            got = on_gpu(gpu, vec, lambda p: dom.fft(kind, p)).reshape(n, t, 12)
            del vec
            assert np.array_equal(got[:, 0, :], S.words(S.periodic_values(0, kind, m, per))), f"periodic, kind {kind}: outputs at multiples of m / n"
            assert not got[:, 1:, :].any(), f"periodic, kind {kind}: an output that is 0 mod r came back non-zero"
            del got
            vec = np.zeros((m, 12), dtype=np.uint64)
            vec[::t] = S.words(stu)
            got = on_gpu(gpu, vec, lambda p: dom.fft(kind, p)).reshape(t, n, 12)
            del vec
            block = S.words(S.stuffed_block(0, kind, m, stu))
            assert np.array_equal(got, np.broadcast_to(block, (t, n, 12))), f"zero-stuffed, kind {kind}"
            del got
    finally:
        if d is not None:
            d.close()
        dom.close()
    print(f"\n[large] 2^{logm}: total {time.time() - t0:.1f} s, of which the oracle's cosetFFT {t2 - t1:.1f} s")


# ---- C: structured inputs through whole kernels ---------------------------------------------------------------------------------
STRUCTURED = [(0, 5), (0, 8), (0, 9), (0, 11), (0, 16), (0, 17), (1, 8), (1, 15)]


def structured_classes(curve, m, seed):
    out = S.classes(curve, m, seed, n=4)
    if m >= 64:
        out += [c for c in S.classes(curve, m, seed + 1, n=16) if c[1][0] in ("periodic", "stuffed")]
    return out


@pytest.mark.parametrize("curve,logm", [pytest.param(c, l, id=case_id(c, l)) for c, l in STRUCTURED])
@pytest.mark.timeout(900)
def test_structured_inputs_four_kinds(gpu, curve, logm):
    """every class of fft_structured through FFT, iFFT, cosetFFT and icosetFFT: the GPU's words, the closed form and the oracle agree"""
    m = 1 << logm
    dom = gpu.Domain(curve, m)
    try:
        for name, spec in structured_classes(curve, m, 50 + logm):
            v = S.words(S.build(curve, m, spec))
            for kind in S.KINDS:
                got = on_gpu(gpu, v, lambda p: dom.fft(kind, p))
                assert np.array_equal(got, O.fft(curve, kind, v).reshape(m, 12)), f"{name}, kind {kind}: against the oracle"
                assert np.array_equal(got, S.words(S.transform(curve, kind, m, spec))), f"{name}, kind {kind}: against the closed form"
    finally:
        dom.close()


@pytest.mark.parametrize("curve,logm", [pytest.param(c, l, id=case_id(c, l)) for c, l in STRUCTURED])
@pytest.mark.timeout(900)
def test_structured_inputs_compute_h_on_satisfied_rows(gpu, curve, logm):
    """cc = ca * cb row by row: A B - C vanishes on the domain, so after the round trip k_h_pointwise works on the coset values of a
    multiple of Z and H has a zero at its top coefficient; for three pairs H is known in closed form.  The row products are Python
    integers (x y / R mod r); a sample of rows is checked against the oracle's own product (field_op 0)."""
    m = 1 << logm
    dom = gpu.Domain(curve, m)
    try:
        for name, sa, sb, closed in S.h_pairs(curve, m, 60 + logm):
            a, b = S.build(curve, m, sa), S.build(curve, m, sb)
            c = S.product_rows(curve, a, b)
            ca, cb, cc = S.words(a), S.words(b), S.words(c)
            for i in sorted({0, 1, 2, 3, m // 2, m - 2, m - 1}):
                assert np.array_equal(O.field_op(curve, 0, ca[i], cb[i]), cc[i]), f"{name}: row {i} is not the oracle's product"
            want = O.compute_h(curve, ca, cb, cc).reshape(m + 1, 12)
            if closed:
                assert np.array_equal(S.words(S.compute_h_closed(curve, m, sa, sb)), want), f"{name}: closed form against the oracle"
            for how, got in zip(("compute_h", "chain x3 + finish", "unfused"), compute_h_three_ways(gpu, dom, curve, ca, cb, cc)):
                assert np.array_equal(got, want), f"{name}: {how}"
    finally:
        dom.close()


STEP_EXT = [(0, D.STEP, 1040), (0, D.STEP, 1536), (1, D.STEP, 1040), (1, D.STEP, 1536), (0, D.STEP, 1025), (1, D.EXTENDED, 1 << 16)]


@pytest.mark.parametrize("curve,kind,m", [pytest.param(c, k, m, id=f"{NAME[c]}-{k}-{m}") for c, k, m in STEP_EXT])
@pytest.mark.timeout(900)
def test_structured_inputs_step_and_extended(gpu, curve, kind, m):
    """constant, delta and all-(r - 1) vectors through the four kinds of a step / extended domain (k_step_pre / k_step_post fold
    big_m / small_m terms per output; k_ext_pre / k_ext_post), whole vector against domain_ref's fast composition, which
    tests/test_domains_cpu.py pins to the definition."""
    r = D.MODULUS[curve]
    assert D.select(curve, m) == (kind, m)
    big = D.step_split(m)[0] if kind == D.STEP else m // 2
    c = S.seeded(curve, 70 + m, 1)[0]
    vectors = [("all-(r-1)", [r - 1] * m), ("const-one", [S.mont_one(curve)] * m), ("const-seeded", [c] * m)]
    for j in sorted({0, m // 2, big - 1, big, m - 1}):
        vectors.append((f"delta-r-1-at-{j}", S.build(curve, m, ("delta", j, r - 1))))
    dom = gpu.Domain.for_size(curve, m)
    try:
        assert (dom.kind, dom.m) == (D.KIND_CODE[kind], m)
        for name, a in vectors:
            v = S.words(a)
            for k, want in ((gpu.FFT, D.fast_fft(curve, kind, m, a)), (gpu.IFFT, D.fast_ifft(curve, kind, m, a)),
                            (gpu.COSET_FFT, D.fast_fft(curve, kind, m, a, True)), (gpu.ICOSET_FFT, D.fast_ifft(curve, kind, m, a, True))):
                got = on_gpu(gpu, v, lambda p: dom.fft(k, p))
                assert np.array_equal(got, S.words(want)), f"{name}, kind {k}"
    finally:
        dom.close()


# ---- k_r1cs_evaluate: rows at the edges of its accumulation ---------------------------------------------------------------------
def edge_system(curve):
    """-> (m, w [m + 1, 12], rows, zero_rows, top_rows): rows as lists of (raw coefficient, variable); the indices of the rows whose
    sum is exactly 0 and of those whose sum is the word pattern r - 1.  Variables 1 ... 200 hold r - 1, 0 is the constant one."""
    r = S.modulus(curve)
    one = S.mont_one(curve)
    sd = S.seeded(curve, 90, 400)
    m = 260
    w = [one] + [r - 1] * 200 + sd[:m - 200]
    w[250] = 0
    w[252] = (r - 1 - w[251]) % r
    cs = sd[100:300]
    neg = lambda x: (r - x) % r
    rows, zero_rows, top_rows = [], [], []

    def add(row, kind=None):
        (zero_rows if kind == "zero" else top_rows if kind == "top" else []).append(len(rows))
        rows.append(row)

    for k in (1, 2, 3, 199, 200):                                        # every coefficient and every variable r - 1
        add([(r - 1, 1 + i) for i in range(k)])
        add([(r - 1, 1)] * k)                                            # ... and the same variable k times
    add([(cs[0], 205), (neg(cs[0]), 205)], "zero")                       # (c, v), (r - c, v)
    add([(cs[0], 205), (cs[1], 206), (neg(cs[0]), 205), (neg(cs[1]), 206)], "zero")
    add([(r - 1, 7), (1, 7)], "zero")                                    # the pair at the edge: r - 1 and 1
    triple = [(cs[2], 207), (cs[3], 207), (neg((cs[2] + cs[3]) % r), 207)]
    add(triple, "zero")                                                  # an odd number of terms: a zero-sum triple
    add([(cs[4], 3), triple[0], (neg(cs[4]), 3), triple[1], triple[2]], "zero")
    pairs = [(cs[i], 1 + i) for i in range(100)]
    add(pairs + [(neg(c), v) for c, v in pairs], "zero")                 # 200 terms summing to 0, the negatives behind all the positives
    add(pairs[:98] + triple + [(neg(c), v) for c, v in pairs[:98]], "zero")     # 199 terms
    add([(one, 1)], "top")                                               # 1 * (r - 1): the sum is the word pattern r - 1
    add([(cs[5], 205), (one, 1), (neg(cs[5]), 205)], "top")
    add([(one, 251), (one, 252)], "top")                                 # x + (r - 1 - x)
    add(pairs[:99] + [(one, 1), (cs[6], 250)] + [(neg(c), v) for c, v in pairs[:99]], "top")     # 200 terms, one of them times zero
    add([(cs[7], 0)])                                                    # the constant column only
    add([(r - 1, 0)])
    add([(one, 0)])
    add([(neg(one), 0), (one, 0)], "zero")
    add([])                                                              # an empty row
    return m, S.words(w), rows, zero_rows, top_rows


def csr(curve, rows):
    rp = np.zeros(len(rows) + 1, dtype=np.uint64)
    rp[1:] = np.cumsum([len(x) for x in rows])
    terms = [t for row in rows for t in row]
    col = np.array([v for _, v in terms], dtype=np.uint32)
    cf = S.words([c for c, _ in terms]) if terms else np.zeros((0, 12), dtype=np.uint64)
    return rp, col, cf


@pytest.mark.parametrize("curve", [0, 1])
def test_r1cs_rows_at_the_edges(gpu, curve):
    """k_r1cs_evaluate sums a row limb-wise and normalises every second term: rows of 1, 2, 3, 199 and 200 terms with every operand
    r - 1, rows that cancel exactly (the result reaches fp_canon as the representative p), rows summing to r - 1, the constant
    column alone; num_inputs 0 and m; out_len exactly nc + num_inputs + 1 and longer.  Against the oracle, and the known sums."""
    m, w, rows, zero_rows, top_rows = edge_system(curve)
    nc = len(rows)
    mats = [csr(curve, rows), csr(curve, rows[::-1]), csr(curve, rows[7:] + rows[:7])]
    top = S.words([S.modulus(curve) - 1])[0]
    dw = gpu.DeviceBuffer.from_numpy(w)
    for num_inputs, extra in ((0, 0), (m, 0), (3, 0), (0, 5), (m, 1)):
        out_len = nc + num_inputs + 1 + extra
        cs = gpu.R1cs(curve, num_inputs, m, nc, mats)
        assert cs.domain_size() == nc + num_inputs + 1
        outs = [gpu.DeviceBuffer.from_numpy(np.full((out_len, 12), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)) for _ in range(3)]
        cs.evaluate(dw.ptr.value, outs[0].ptr.value, outs[1].ptr.value, outs[2].ptr.value, out_len)
        got = [o.to_numpy().reshape(out_len, 12) for o in outs]
        want = O.r1cs_evaluate(curve, num_inputs, nc, mats, w, out_len)
        for k in range(3):
            assert np.array_equal(got[k], want[k]), f"matrix {k}, num_inputs {num_inputs}, out_len {out_len}"
        assert not got[0][zero_rows].any(), "a row that cancels exactly is not all-zero words"
        assert all(np.array_equal(got[0][i], top) for i in top_rows), "a row summing to r - 1"
        assert np.array_equal(got[0][nc:nc + num_inputs + 1], w[:num_inputs + 1])
        assert not got[0][nc + num_inputs + 1:].any() and not got[1][nc:].any() and not got[2][nc:].any()
        for o in outs:
            o.close()
        cs.close()
    dw.close()


# ---- element-wise vector kernels -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_vector_ops_edges_and_aliased_operands(gpu, curve, n):
    """vec_muleq / vec_subeq / vec_scale around the block size, operands 0, one and r - 1, b equal to a by value and -- as the
    reference's vector_Fr_muleq loop allows -- dev_a and dev_b the SAME pointer (square in place, subtract to zero)."""
    r = S.modulus(curve)
    one = S.mont_one(curve)
    edges = [0, one, r - 1, r - one]
    fop = lambda op, x, y: np.stack([O.field_op(curve, op, p, q) for p, q in zip(x, y)])
    variants = [([e], [f]) for e in edges for f in edges] if n == 1 else [None]
    for var in variants:
        if var:
            a, b = S.words(var[0]), S.words(var[1])
        else:
            ai, bi = S.seeded(curve, 80 + n, n), S.seeded(curve, 81 + n, n)
            ai[:4], bi[:4] = edges, [r - 1] * 4
            ai[8:12], bi[8:12] = [r - 1] * 4, edges
            ai[n - 1], bi[n - 1], bi[n - 2] = r - 1, r - 1, 0
            a, b = S.words(ai), S.words(bi)
        da, db = gpu.DeviceBuffer.from_numpy(a), gpu.DeviceBuffer.from_numpy(b)
        gpu.vec_muleq(curve, da.ptr.value, db.ptr.value, n)
        prod = fop(0, a, b)
        assert np.array_equal(da.to_numpy().reshape(n, 12), prod), "muleq"
        gpu.vec_subeq(curve, da.ptr.value, db.ptr.value, n)
        assert np.array_equal(da.to_numpy().reshape(n, 12), fop(2, prod, b)), "subeq"
        assert np.array_equal(db.to_numpy().reshape(n, 12), b), "the second operand changed"
        da.close()
        # b = a by value
        da, dc = gpu.DeviceBuffer.from_numpy(a), gpu.DeviceBuffer.from_numpy(a)
        gpu.vec_muleq(curve, da.ptr.value, dc.ptr.value, n)
        sq = fop(0, a, a)
        assert np.array_equal(da.to_numpy().reshape(n, 12), sq), "muleq, b = a by value"
        gpu.vec_subeq(curve, dc.ptr.value, da.ptr.value, n)              # a - a^2
        assert np.array_equal(dc.to_numpy().reshape(n, 12), fop(2, a, sq)), "subeq a - a^2"
        dc.close(); dc = gpu.DeviceBuffer.from_numpy(sq)
        gpu.vec_subeq(curve, da.ptr.value, dc.ptr.value, n)              # equal by value: zeros
        assert not da.to_numpy().any(), "subeq, b = a by value"
        da.close(); dc.close()
        # dev_a == dev_b: the same pointer
        da = gpu.DeviceBuffer.from_numpy(a)
        gpu.vec_muleq(curve, da.ptr.value, da.ptr.value, n)
        assert np.array_equal(da.to_numpy().reshape(n, 12), sq), "muleq, dev_a == dev_b"
        gpu.vec_subeq(curve, da.ptr.value, da.ptr.value, n)
        assert not da.to_numpy().any(), "subeq, dev_a == dev_b"
        da.close()
        # vec_scale, out of place and in place, by 0, one, r - 1 and a seeded factor
        for kv in edges[:3] + S.seeded(curve, 82, 1):
            k = S.words([kv])[0]
            want = np.stack([O.field_op(curve, 0, x, k) for x in b])
            dd = gpu.DeviceBuffer.from_numpy(np.full((n, 12), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64))
            gpu.vec_scale(curve, dd.ptr.value, db.ptr.value, k, n)
            assert np.array_equal(dd.to_numpy().reshape(n, 12), want), "scale"
            assert np.array_equal(db.to_numpy().reshape(n, 12), b), "scale changed its source"
            dd.close(); dd = gpu.DeviceBuffer.from_numpy(b)
            gpu.vec_scale(curve, dd.ptr.value, dd.ptr.value, k, n)
            assert np.array_equal(dd.to_numpy().reshape(n, 12), want), "scale in place"
            dd.close()
        db.close()
