"""GPU: fixed-base batch scalar multiplication (FixedBase / mnt753_batch_exp) on both curves and both groups.

Expected values (tests/batch_exp_ref.py): (a) libff-minted goldens, (b) the oracle's scalar multiplication per value (cached per
(curve, group)), (c) the MSM fold for everything bulk.  Small widths and a tile of two inversion runs put every edge -- the extreme
digits of every window, the carry into the top window, a tile boundary, a partial inversion run, identity outputs inside a run,
an accumulator that equals its row -- within a few hundred scalars."""
import ctypes

import numpy as np
import pytest

import batch_exp_ref as BR
import domain_ref as D
import golden_io as G
import msm_structured as S
import oracle_lib as O

pytestmark = pytest.mark.gpu

GROUPS = [(0, 1), (0, 2), (1, 1), (1, 2)]
G1_WIDTHS = tuple(range(2, 13))
G2_WIDTHS = (3, 4, 7, 12)
STRUCTURED = [(c, g, w) for c, g in GROUPS for w in (G1_WIDTHS if g == 1 else G2_WIDTHS)]
# the wrap scalars put their k on the top window's boundary at widths 5, 6, 7, 10, 11, 15, 17 and 22 (test_batch_exp_cpu.py); run here at
# those whose table stays below 1 GB (width 22: 19 GB of G1 rows, 49 GB on MNT6753 G2 -- nothing for a shared device)
WRAP = [(c, g, w) for c, g in GROUPS for w in ((5, 6, 7, 10, 11, 15, 17) if g == 1 else (5, 7, 11))]
_GEN = {}


def generator(gpu, curve, group):
    if (curve, group) not in _GEN:
        g = gpu.api.test_generator(curve, group)
        g.setflags(write=False)
        _GEN[(curve, group)] = g
    return _GEN[(curve, group)]


def run(gpu, curve, group, point, ints, window_bits=0, tile=0, coeff=None):
    fb = gpu.FixedBase(curve, group, point, window_bits=window_bits, tile=tile)
    try:
        return fb.batch_exp(BR.wire(curve, ints), coeff=None if coeff is None else BR.wire(curve, [coeff])[0]), fb.plan()
    finally:
        fb.close()


def check_direct(curve, group, point, ints, outs, what):
    bad = [hex(s) for s, o in zip(ints, outs) if not np.array_equal(o, BR.oracle_scale(curve, group, point, s))]
    assert not bad, f"{what}: {len(bad)} of {len(ints)} outputs differ from the oracle, first {bad[:3]}"


# ---- (a) goldens -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [4, 0], ids=["w4", "default"])
@pytest.mark.parametrize("curve,group", GROUPS)
def test_libff_goldens(gpu, curve, group, width):
    """every P, s, s P record libff minted (golden_io.group: 8 per group; golden_io.msm with one base), the base being the golden's P"""
    recs = [(g["P"], g["s"], g["mul"]) for g in G.group(curve, group)]
    b, s, res = G.msm(curve, group, 1)
    recs.append((b[0], s[0], res))
    for k, (P, s, mul) in enumerate(recs):
        fb = gpu.FixedBase(curve, group, P, window_bits=width)
        try:
            got = fb.batch_exp(np.stack([s, s]))
            plan = fb.plan()
        finally:
            fb.close()
        assert plan["window_bits"] == (width or plan["window_bits"]) and plan["windows"] == S.windows(plan["window_bits"])
        assert np.array_equal(got[0], mul) and np.array_equal(got[1], mul), f"golden record {k} at width {plan['window_bits']}"


# ---- structured scalars --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve,group,width", STRUCTURED)
def test_structured_scalars_at_every_width(gpu, curve, group, width):
    """extremes, carry chains, field edges and every row of window 0 (dense), behind the anchors 0, 1, 2, r - 1, r - 2, 2^752 and the
    top-window extremes of every tested width: the anchors against the oracle value by value, everything by the fold"""
    P = generator(gpu, curve, group)
    anchors = BR.anchors(curve, G1_WIDTHS)
    ints = list(anchors)
    for _, fam in BR.structured(curve, width):
        ints += fam
    outs, plan = run(gpu, curve, group, P, ints, window_bits=width, tile=256)
    assert plan["window_bits"] == width and plan["tile"] == 256
    assert not outs[0].any(), "scalar 0 must give the identity (all words zero)"
    check_direct(curve, group, P, anchors, outs[:len(anchors)], f"anchors, width {width}")
    BR.fold_check(gpu, curve, group, P, ints, outs, 5100 + width, f"structured, curve {curve} group {group} width {width}")


@pytest.mark.parametrize("width", [5, 11])
@pytest.mark.parametrize("curve,group", GROUPS)
def test_single_bits(gpu, curve, group, width):
    """2^k for every bit position: every straddle of a 32-bit word by a window"""
    P = generator(gpu, curve, group)
    ints = S.single_bits(curve)
    outs, _ = run(gpu, curve, group, P, ints, window_bits=width, tile=512)
    BR.fold_check(gpu, curve, group, P, ints, outs, 5200 + width, f"single bits, curve {curve} group {group} width {width}")


# ---- wrap scalars ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve,group,width", WRAP)
def test_wrap_scalars_meet_an_accumulator_equal_to_its_row(gpu, curve, group, width):
    """s_k = 2 floor(r / 2^k) 2^k - r: the partial sum below bit k and the row of the digits above it are the same point; every value
    against the oracle (at most 53 per curve)"""
    P = generator(gpu, curve, group)
    fam = BR.wrap_family(curve)
    assert any(k == (S.windows(width) - 1) * width for k, _ in fam), "no member on this width's top-window boundary"
    ints = [s for _, s in fam]
    # (the default tile: the table of the wide widths is built in pieces of a tile, millions of rows)
    outs, _ = run(gpu, curve, group, P, ints, window_bits=width)
    check_direct(curve, group, P, ints, outs, f"wrap scalars, width {width}")


# ---- shapes ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve,group", GROUPS)
def test_shapes_tiles_and_identity_outputs(gpu, curve, group):
    """tile = 2 B: n around one inversion run, one tile and several; zeros (identity outputs) first, last, through one whole inversion
    run and isolated; repeated scalars"""
    P = generator(gpu, curve, group)
    r = BR.modulus(curve)
    probe = gpu.FixedBase(curve, group, P, window_bits=6, tile=1)
    B = probe.plan()["inversion_batch"]
    assert probe.plan()["tile"] == B and probe.table_bytes > 0
    probe.close()
    fb = gpu.FixedBase(curve, group, P, window_bits=6, tile=2 * B)
    try:
        assert fb.plan()["tile"] == 2 * B
        uniform = D.from_wire(curve, gpu.synth_scalars(curve, 77, 6 * B + 1))
        for n in (0, 1, B - 1, B, B + 1, 2 * B, 2 * B + 1, 6 * B + 1):
            ints = list(uniform[:n])
            zeros = set()
            if n > 2:
                zeros |= {0, n - 1}
            if n > 2 * B:
                zeros |= set(range(B, 2 * B))
            if n > 3 * B + 5:
                zeros |= {3 * B + 5, 3 * B + 7}
            for z in zeros:
                ints[z] = 0
            if n > 4 * B + 2:
                ints[4 * B + 1] = ints[4 * B + 2] = ints[2]
                ints[5 * B] = r - ints[2]
            outs = fb.batch_exp(BR.wire(curve, ints))
            assert outs.shape == (n, O.aff_words(curve, group))
            for z in zeros:
                assert not outs[z].any(), f"n = {n}: output {z} of scalar 0 is not the identity"
            assert all(outs[k].any() for k in range(n) if k not in zeros), f"n = {n}: an identity where the scalar is not 0"
            if n > 4 * B + 2:
                assert np.array_equal(outs[4 * B + 1], outs[2]) and np.array_equal(outs[4 * B + 2], outs[2])
            BR.fold_check(gpu, curve, group, P, ints, outs, 5300 + n, f"shapes, curve {curve} group {group} n = {n}")
    finally:
        fb.close()


# ---- symmetry ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve,group", GROUPS)
def test_negated_scalar_gives_negated_point(gpu, curve, group):
    P = generator(gpu, curve, group)
    r = BR.modulus(curve)
    s = [v for v in D.from_wire(curve, gpu.synth_scalars(curve, 78, 24)) if v] + [1, 2, 1 << 752]
    outs, _ = run(gpu, curve, group, P, s + [r - v for v in s], window_bits=7, tile=32)
    for k in range(len(s)):
        assert np.array_equal(outs[len(s) + k], BR.neg_point(curve, group, outs[k])), f"scalar {hex(s[k])}"


# ---- coefficient ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve,group", GROUPS)
def test_coefficient(gpu, curve, group):
    """batch_exp_with_coeff: coeff in {1, 0, r - 1, uniform} against the scalars multiplied in Python integers; no coefficient == 1"""
    P = generator(gpu, curve, group)
    r = BR.modulus(curve)
    s = D.from_wire(curve, gpu.synth_scalars(curve, 79, 40)) + [0, 1, r - 1]
    fb = gpu.FixedBase(curve, group, P, window_bits=8, tile=32)
    try:
        plain = fb.batch_exp(BR.wire(curve, s))
        for coeff in (1, 0, r - 1, D.from_wire(curve, gpu.synth_scalars(curve, 80, 1))[0]):
            got = fb.batch_exp(BR.wire(curve, s), coeff=BR.wire(curve, [coeff])[0])
            exp = fb.batch_exp(BR.wire(curve, [coeff * v % r for v in s]))
            assert np.array_equal(got, exp), f"coeff {hex(coeff)}"
            if coeff == 1:
                assert np.array_equal(got, plain)
            if coeff == 0:
                assert not got.any()
        BR.fold_check(gpu, curve, group, P, s, plain, 5400, f"coefficient base run, curve {curve} group {group}")
    finally:
        fb.close()


# ---- ends ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve,group", GROUPS)
def test_host_and_device_ends(gpu, curve, group):
    """the four host / device combinations of scalars and output give the same words; a device output feeds a base set directly; the
    caller's scalars are unchanged after a call with a coefficient"""
    P = generator(gpu, curve, group)
    r = BR.modulus(curve)
    n, aw = 70, O.aff_words(curve, group)
    s = D.from_wire(curve, gpu.synth_scalars(curve, 81, n))
    s[5] = 0
    sw = BR.wire(curve, s)
    coeff = D.from_wire(curve, gpu.synth_scalars(curve, 82, 1))[0]
    cw = BR.wire(curve, [coeff])[0]
    fb = gpu.FixedBase(curve, group, P, window_bits=9, tile=32)
    d_s = gpu.DeviceBuffer.from_numpy(sw)
    d_o = gpu.DeviceBuffer(8 * aw * n)
    try:
        hh = fb.batch_exp(sw, coeff=cw)
        assert np.array_equal(sw, BR.wire(curve, s)), "host scalars were written"
        dh = fb.batch_exp(d_s.ptr.value, coeff=cw, on_device=True, n=n)
        assert fb.batch_exp(sw, coeff=cw, out_ptr=d_o.ptr.value) is None
        hd = d_o.to_numpy().reshape(n, aw)
        gpu.lib().mnt753_dev_memset(d_o.ptr, 0xff, d_o.nbytes)
        assert fb.batch_exp(d_s.ptr.value, coeff=cw, on_device=True, n=n, out_ptr=d_o.ptr.value) is None
        gpu.lib().mnt753_sync(None)
        dd = d_o.to_numpy().reshape(n, aw)
        assert np.array_equal(d_s.to_numpy().reshape(n, 12), sw), "device scalars were written"
        assert np.array_equal(hh, dh) and np.array_equal(hh, hd) and np.array_equal(hh, dd)
        BR.fold_check(gpu, curve, group, P, [coeff * v % r for v in s], hh, 5500, f"ends, curve {curve} group {group}")
        # the device output as a base set, without a round trip
        sk = gpu.synth_scalars(curve, 83, n)
        bs = gpu.BaseSet(curve, group, d_o.ptr.value, on_device=True, n=n)
        try:
            got = gpu.point_to_affine(curve, group, bs.msm(sk))
        finally:
            bs.close()
        total = sum(a * coeff * e for a, e in zip(D.from_wire(curve, sk), s)) % r
        assert np.array_equal(got, BR.oracle_scale(curve, group, P, total))
        # overlapping ends are refused
        rc = gpu.lib().mnt753_batch_exp(fb._h, d_s.ptr, 1, n, None, d_s.ptr, 1, None)
        assert rc == -1 and b"overlap" in gpu.lib().mnt753_last_error()
    finally:
        fb.close(); d_s.close(); d_o.close()


# ---- bases -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve,group", GROUPS)
def test_other_bases(gpu, curve, group):
    """the identity base gives all zeros (no table is read); -G and a golden P by the fold and the oracle"""
    r = BR.modulus(curve)
    aw = O.aff_words(curve, group)
    s = D.from_wire(curve, gpu.synth_scalars(curve, 84, 37)) + [0, 1, r - 1]
    outs, _ = run(gpu, curve, group, np.zeros(aw, dtype=np.uint64), s, window_bits=5, tile=16)
    assert outs.shape == (len(s), aw) and not outs.any()
    ident_x = np.array(generator(gpu, curve, group))
    ident_x[aw // 2:] = 0                       # y == 0 is the identity whatever x holds
    outs, _ = run(gpu, curve, group, ident_x, s, window_bits=5, tile=16)
    assert not outs.any()
    for name, P in (("-G", BR.neg_point(curve, group, generator(gpu, curve, group))), ("golden P", G.group(curve, group)[3]["P"])):
        outs, _ = run(gpu, curve, group, P, s, window_bits=5, tile=16)
        check_direct(curve, group, P, [1, r - 1], outs[-2:], name)
        BR.fold_check(gpu, curve, group, P, s, outs, 5600, f"base {name}, curve {curve} group {group}")


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals(gpu):
    L = gpu.lib()
    h = ctypes.c_void_p()
    g = generator(gpu, 0, 1)
    p = ctypes.c_void_p(g.ctypes.data)
    for what, args in (("width 1", (0, 1, p, 1, 0)), ("width above the cap", (0, 1, p, 23, 0)), ("curve 2", (2, 1, p, 4, 0)), ("group 3", (0, 3, p, 4, 0)),
                       ("null point", (0, 1, None, 4, 0))):
        assert L.mnt753_fixed_base_create(*args, ctypes.byref(h)) == -1, what
        assert L.mnt753_last_error().startswith(b"fixed_base_create"), what
        assert not h.value
    fb = gpu.FixedBase(0, 1, g, window_bits=4, tile=16)
    try:
        assert L.mnt753_batch_exp(fb._h, None, 0, 3, None, p, 0, None) == -1
        assert fb.batch_exp(np.zeros((0, 12), dtype=np.uint64)).shape == (0, 24)       # n = 0 succeeds and writes nothing
        assert L.mnt753_batch_exp(fb._h, None, 0, 0, None, None, 0, None) == 0
    finally:
        fb.close()
