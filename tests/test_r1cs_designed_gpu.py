"""GPU: k_r1cs_evaluate, k_qap_chunks and k_qap_fold on the designed systems of tests/r1cs_designed.py -- sums that are = 0, = 1 and
= r - 1 (mod r), operands at the edges of the wire range, rows of 1 .. 5, 200 and 201 terms of the largest pair, waves of mixed length,
nc = 0, an empty matrix, num_inputs = 0 and m, chunk partials that cancel only in the fold, a cancelled seed, t inside the domain.
Every comparison is exact words against the integer model, which tests/test_r1cs_designed_cpu.py pins to the oracle and to
qap_ref.instance_map."""
import numpy as np
import pytest

import domain_ref as D
import qap_ref as Q
import r1cs_designed as RD
import validate_ref as V

pytestmark = pytest.mark.gpu

PATTERN = 0xA5A5A5A5A5A5A5A5                      # above r in every element: never a value the kernels write
GUARD = 3                                         # rows behind every output that must keep the pattern
DOMAINS = {0: (D.BASIC, 1024), 1: (Q.MIXED, 640)}  # the smallest basic / mixed domains that hold 2 L + 2 rows and the inputs at L = 256


def make_cs(gpu, system):
    return gpu.R1cs(system.curve, system.num_inputs, system.m, system.nc, RD.matrices(system))


def evaluate_into_pattern(gpu, cs, dw, out_len):
    """ca, cb, cc evaluated into buffers of out_len + GUARD rows pre-filled with the pattern -> three [out_len, 12] arrays; nothing
    beyond out_len is written"""
    rows = out_len + GUARD
    bufs = [gpu.DeviceBuffer.from_numpy(np.full(12 * rows, PATTERN, dtype=np.uint64)) for _ in range(3)]
    cs.evaluate(dw.ptr.value, bufs[0].ptr.value, bufs[1].ptr.value, bufs[2].ptr.value, out_len)
    gpu.lib().mnt753_sync(None)
    out = [b.to_numpy().reshape(rows, 12) for b in bufs]
    for b in bufs:
        b.close()
    for k, o in enumerate(out):
        assert (o[out_len:] == PATTERN).all(), f"matrix {k}: written beyond out_len"
    return [o[:out_len] for o in out]


def assert_rows(got, want, what):
    """exact words, every row below out_len written; on a difference, name the first rows"""
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape
        diff = np.flatnonzero((g != w).any(axis=1))
        assert diff.size == 0, f"{what}: matrix {k}, {diff.size} rows differ, first {diff[:8].tolist()}"


@pytest.mark.parametrize("curve", [0, 1])
def test_evaluate_on_the_designed_system(gpu, curve):
    system, info = RD.designed_system(curve)
    out_len = system.nc + system.num_inputs + 1 + 9
    cs = make_cs(gpu, system)
    dw = gpu.DeviceBuffer.from_numpy(RD.witness_words(system))
    want = RD.evaluate_words(system, out_len)
    got = evaluate_into_pattern(gpu, cs, dw, out_len)
    assert_rows(got, want, "designed system")
    for cls in ("zero2", "zero3", "zero8", "empty"):                     # a sum = 0 is 24 zero words, not the words of r
        assert not got[0][info[cls]].any(), cls
    assert_rows(evaluate_into_pattern(gpu, cs, dw, out_len), want, "second evaluation")
    cs.close(); dw.close()


@pytest.mark.parametrize("curve", [0, 1])
def test_evaluate_on_every_shape(gpu, curve):
    for name, system, out_len in RD.shapes(curve):
        cs = make_cs(gpu, system)
        assert cs.domain_size() == system.nc + system.num_inputs + 1
        dw = gpu.DeviceBuffer.from_numpy(RD.witness_words(system))
        assert_rows(evaluate_into_pattern(gpu, cs, dw, out_len), RD.evaluate_words(system, out_len), name)
        cs.close(); dw.close()


@pytest.mark.parametrize("curve", [0, 1])
def test_evaluate_after_swap_ab(gpu, curve):
    system = RD.swap_system(curve)
    out_len = system.nc + system.num_inputs + 1
    cs = make_cs(gpu, system)
    dw = gpu.DeviceBuffer.from_numpy(RD.witness_words(system))
    assert_rows(evaluate_into_pattern(gpu, cs, dw, out_len), RD.evaluate_words(system, out_len), "before the swap")
    assert cs.swap_ab_if_beneficial() and cs.swapped
    want = RD.evaluate_words(RD.swapped(system), out_len)
    assert_rows(evaluate_into_pattern(gpu, cs, dw, out_len), want, "after the swap")
    assert_rows(evaluate_into_pattern(gpu, cs, dw, out_len), want, "after the swap, again")
    assert not cs.swap_ab_if_beneficial() and cs.swapped                 # a now touches more variables than b
    cs.close(); dw.close()


@pytest.mark.parametrize("curve", [0, 1])
def test_check_on_the_satisfied_variant_and_on_disturbed_rows(gpu, curve):
    system, _, disturb = RD.satisfied_system(curve)
    dw = gpu.DeviceBuffer.from_numpy(RD.witness_words(system))
    cs = make_cs(gpu, system)
    assert cs.check(dw.ptr.value) == (0, 0, 0)
    cs.close()
    first, mid, last = disturb
    for changed in ((first,), (mid,), (last,), (mid, last), (first, mid, last)):
        cs = make_cs(gpu, RD.disturbed(system, changed))
        assert cs.check(dw.ptr.value) == (len(changed), min(changed), V.UNSATISFIED), changed
        cs.close()
    dw.close()


# ---- the QAP column sums ------------------------------------------------------------------------------------------------------------
def make_domain(gpu, curve):
    kind, dm = DOMAINS[curve]
    dom = gpu.Domain(curve, dm) if kind == D.BASIC else gpu.Domain.mixed(curve, dm)
    assert dom.m == dm and dom.kind == Q.KIND_CODE[kind]
    return dom, kind, dm


def chunk_terms(gpu, curve):
    full, _ = RD.designed_system(curve)
    probe = make_cs(gpu, full)
    L = probe.qap_plan()["chunk_terms"]
    probe.close()
    return L


def qap_into_pattern(gpu, cs, dom, t):
    """At, Bt, Ct (m + 1 elements) and Ht (dom.m + 1) into one pattern-filled buffer with guard rows behind each -> four arrays and Zt"""
    nv, nh = cs.m + 1, dom.m + 1
    sizes = [nv, nv, nv, nh]
    starts = np.cumsum([0] + [n + GUARD for n in sizes])
    buf = gpu.DeviceBuffer.from_numpy(np.full(12 * int(starts[-1]), PATTERN, dtype=np.uint64))
    out = [buf.ptr.value + 96 * int(s) for s in starts[:4]]
    zt = cs.qap_at(dom, D.to_wire(cs.curve, [t])[0], out=out)[4]
    gpu.lib().mnt753_sync(None)
    raw = buf.to_numpy().reshape(-1, 12)
    buf.close()
    got = []
    for s, n in zip(starts, sizes):
        assert (raw[int(s) + n:int(s) + n + GUARD] == PATTERN).all(), "written beyond the output"
        got.append(raw[int(s):int(s) + n].copy())
    return got, zt


def assert_qap(gpu, cs, dom, kind, qs, t, want_abc, what):
    curve, r = qs.curve, D.MODULUS[qs.curve]
    got, zt = qap_into_pattern(gpu, cs, dom, t)
    assert_rows(got[:3], [D.to_wire(curve, v) for v in want_abc], what)
    assert_rows(got[3:], [D.to_wire(curve, [pow(t, i, r) for i in range(dom.m + 1)])], what + ": Ht")
    assert zt.tolist() == D.to_wire(curve, [Q.vanishing(curve, kind, dom.m, t)])[0].tolist(), what + ": Zt"
    return got


@pytest.mark.parametrize("curve", [0, 1])
def test_qap_at_on_designed_columns(gpu, curve):
    """chunk partials that are each non-zero and cancel in the fold (with and without the seed), the cancelled seed, the seed alone, a
    chunk whose own partial is = 0, designed coefficients; then the same system with no term at all and with b alone empty"""
    dom, kind, dm = make_domain(gpu, curve)
    L = chunk_terms(gpu, curve)
    t = int.from_bytes(np.random.default_rng(92 + curve).bytes(96), "little") % D.MODULUS[curve]
    u = Q.lagrange_fast(curve, kind, dm, t)
    qs = RD.qap_system(curve, L, u)
    assert qs.nc + qs.num_inputs + 1 <= dm
    for empty in ((), (0, 1, 2), (1,)):
        variant = RD.qap_variant(qs, empty)
        cs = make_cs(gpu, variant)
        plan = cs.qap_plan()
        assert plan["chunk_terms"] == L
        if not empty:
            assert plan["split_columns"] == len(qs.classes["split"]) == 9 and plan["longest_column"] == 2 * L + 1
        if len(empty) == 3:
            assert plan["work_items"] == 0 and plan["terms"] == 0
        want = RD.qap_model(variant, u, check_classes=not empty)
        got = assert_qap(gpu, cs, dom, kind, variant, t, want, f"empty {empty}")
        if not empty:
            for which, col in RD.zero_columns(qs):                         # 24 zero words, not the words of r
                assert not got[which][col].any(), (which, col)
            assert got[0][1].tolist() == D.to_wire(curve, [u[qs.nc + 1]])[0].tolist()
        else:
            for k in empty:
                if k:
                    assert not got[k].any()
            if 0 in empty:
                assert_rows([got[0][:qs.num_inputs + 1]], [D.to_wire(curve, u[qs.nc:qs.nc + qs.num_inputs + 1])], "the seeds")
                assert not got[0][qs.num_inputs + 1:].any()
        again, _ = qap_into_pattern(gpu, cs, dom, t)                       # a second call on the kept view gives the same words
        assert_rows(again, got, "second call")
        cs.close()
    dom.close()


@pytest.mark.parametrize("curve", [0, 1])
def test_qap_at_with_t_inside_the_domain(gpu, curve):
    """t = the j-th domain element: u is 1 at j and 0 elsewhere, so every product but one has a zero operand.  j below nc (in the
    first, second and third chunk of the long columns), j = nc + i at both ends of the inputs, j beyond both."""
    dom, kind, dm = make_domain(gpu, curve)
    L = chunk_terms(gpu, curve)
    qs = RD.qap_system(curve, L)
    cs = make_cs(gpu, qs)
    for j in RD.inside_indices(qs, dm):
        t = D.element(curve, Q._dkind(kind), dm, j)
        want = RD.row_coefficients(qs, j)
        assert want == RD.qap_model(qs, RD.indicator(dm, j), check_classes=False)
        got = assert_qap(gpu, cs, dom, kind, qs, t, want, f"t = element {j}")
        if j > qs.nc + qs.num_inputs:
            assert not any(g.any() for g in got[:3])
    cs.close(); dom.close()
