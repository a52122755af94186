"""GPU: the MSM's digit extraction on the structured scalars of tests/msm_structured.py -- a single bit at every position, the extreme
digit +-2^(c-1) in every window, carry chains, the ends of the field, every bucket occupied -- through each of its three copies
(MNT753_MSM_SORT = atomic: k_scalar_digits over lds_bits; generic: k_part_pass over booth_digit; part: k_part_pass_c<., C, .> over
reg_bits<C> for C = 14 .. 22, k_part_pass below that) at every table width 12 .. 22, without the table at widths from 3 to 20, on
G1 and on the lane-split G2 kernels of both curves.  Every comparison is a bit-exact group element.

The bases are synthetic points with known discrete logs: the expected value of a family is (sum_k s_k e_k mod r) G
(synth_expected_msm), computed once per (curve, group, family) -- it does not depend on the width or the sort stage -- and
tests/test_msm_structured_cpu.py pins that expectation to the oracle's multi-exp on the host.  One base set holds all families behind
each other and each family is an MSM of its own through base_offset, so a failure names the family, the width and the sort stage.

(The sort stage is a request: where the partition passes cannot stage a plan in LDS -- W = 95 windows at c = 8 -- the library takes
the atomic sort whatever MNT753_MSM_SORT says, which is why c = 8 is listed under "atomic" alone.)"""
import json
import os
import subprocess

import numpy as np
import pytest

import domain_ref as D
import msm_structured as S
import oracle_lib as O

pytestmark = pytest.mark.gpu

CURVES = [0, 1]
SORTS = ("part", "generic", "atomic")
G1_FAMILIES = ("single_bits", "edges", "extremes", "carry_chains")
N_POINTS = {1: 1600, 2: 400}
_POINTS, _EXPECT = {}, {}


def base_seed(curve, group):
    return 9400 + 10 * curve + group


def frozen(a):
    a.setflags(write=False)
    return a


def points(gpu, curve, group, seed=None, n=None):
    """the synthetic bases of (curve, group): one array per module run, shared and read-only"""
    seed = base_seed(curve, group) if seed is None else seed
    n = N_POINTS[group] if n is None else n
    key = (curve, group, seed, n)
    if key not in _POINTS:
        _POINTS[key] = frozen(gpu.synth_points(curve, group, seed, n))
    return _POINTS[key]


def expected(gpu, curve, group, seed, name, offset, ints):
    """affine words of sum_k ints[k] * base[offset + k] through the discrete logs of the bases; cached per family"""
    key = (curve, group, seed, name, offset)
    if key not in _EXPECT:
        sc = np.zeros((offset + len(ints), 12), dtype=np.uint64)
        sc[offset:] = S.wire(curve, ints)
        _EXPECT[key] = frozen(gpu.point_to_affine(curve, group, gpu.synth_expected_msm(curve, group, seed, sc)))
    return _EXPECT[key]


def layout(curve, c, names):
    """[(label, offset, integers)]: the families behind each other; the width-independent ones first, so that their offsets (and
    their cached expectations) are the same at every width"""
    out, off = [], 0
    for name in names:
        ints = S.single_bits(curve)[::4] if name == "single_bits/4" else S.family(curve, name, c)
        out.append((name if name == "single_bits/4" else S.label(name, c), off, ints))
        off += len(ints)
    assert off <= N_POINTS[2 if "single_bits/4" in names else 1]
    return out, off


def run_families(gpu, curve, group, bs, fams, what):
    """one MSM per family; every family runs, the failure lists all that differ"""
    seed = base_seed(curve, group)
    bad = []
    for name, off, ints in fams:
        got = gpu.point_to_affine(curve, group, bs.msm(S.wire(curve, ints), base_offset=off))
        if not np.array_equal(got, expected(gpu, curve, group, seed, name, off, ints)):
            bad.append(name)
    assert not bad, f"{what}: wrong group element on {bad}"


# ---- a. the conversion in front of every extractor --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mod", [0, 1])
def test_wire_to_integer_on_every_family_scalar(gpu, mod):
    """fp_wire_to_integer alone (test hook op 4, as_bigint on the device) on every scalar any test of this module feeds the MSM, for
    both moduli (modulus A is Fr of MNT4753, B of MNT6753): the 24 words the three extractors slice are the integer"""
    curve = mod
    ints = set(S.single_bits(curve)) | set(S.edges(curve)) | set(S.dense(curve, 8)) | set(S.dense(curve, 12)) | {0}
    for c in S.WIDTHS:
        ints |= set(S.extremes(curve, c)) | set(S.carry_chains(curve, c))
    ints = sorted(ints)
    got = D.mont_ints(gpu.api.test_field_op(mod, 4, S.wire(curve, ints)))
    bad = [hex(s) for s, g in zip(ints, got) if s != g]
    assert not bad, f"{len(bad)} of {len(ints)} scalars converted wrongly, first {bad[:3]}"


# ---- b. every extractor at every table width ------------------------------------------------------------------------------------------------
TABLE_CASES = [(c, sort) for c in range(12, 23) for sort in SORTS] + [(8, "atomic")]


@pytest.mark.parametrize("c,sort", TABLE_CASES)
@pytest.mark.parametrize("curve", CURVES)
def test_table_mode_at_every_width_and_sort_stage(gpu, curve, c, sort, monkeypatch):
    """One bucket set shared by all windows (the window table): the extreme digit is the set's last bucket, key nb - 1.  G1, both scalar
    fields, c = 12 .. 22 under each sort stage, and c = 8 (atomic) with every bucket of the set occupied as a fifth family."""
    monkeypatch.setenv("MNT753_MSM_PRECOMP", "1")
    monkeypatch.setenv("MNT753_MSM_TABLE_BITS", str(c))
    monkeypatch.setenv("MNT753_MSM_SORT", sort)
    fams, total = layout(curve, c, G1_FAMILIES + (("dense",) if c == 8 else ()))
    bs = gpu.BaseSet(curve, 1, points(gpu, curve, 1)[:total])
    try:
        gpu.point_to_affine(curve, 1, bs.msm(S.wire(curve, [1])))
        plan = gpu.msm_last_plan()
        assert plan["window_table"] and plan["window_bits"] == c and plan["windows"] == S.windows(c), plan
        run_families(gpu, curve, 1, bs, fams, f"curve {curve}, table, c = {c}, sort {sort}")
    finally:
        bs.close()


# ---- c. one bucket set per window ---------------------------------------------------------------------------------------------------------
NO_TABLE_CASES = [(3, "atomic"), (7, "atomic"), (11, "atomic"), (16, "atomic"), (20, "atomic"), (16, "part"), (16, "generic")]


@pytest.mark.parametrize("c,sort", NO_TABLE_CASES)
@pytest.mark.parametrize("curve", CURVES)
def test_without_the_table(gpu, curve, c, sort, monkeypatch):
    """W bucket sets: key = w * nb + |d| - 1.  c = 3 divides 753: the top window holds carries only (W = 252 exists for it).  c = 16
    under the partition passes: 48 sets of 2^15 buckets = 1536 partitions, a window's last key next to the following window's first."""
    monkeypatch.setenv("MNT753_MSM_PRECOMP", "0")
    monkeypatch.setenv("MNT753_MSM_SORT", sort)
    fams, total = layout(curve, c, G1_FAMILIES)
    old = gpu.lib().mnt753_msm_set_window_bits(c)
    try:
        bs = gpu.BaseSet(curve, 1, points(gpu, curve, 1)[:total])
        try:
            gpu.point_to_affine(curve, 1, bs.msm(S.wire(curve, [1])))
            plan = gpu.msm_last_plan()
            assert not plan["window_table"] and plan["window_bits"] == c and plan["windows"] == S.windows(c), plan
            run_families(gpu, curve, 1, bs, fams, f"curve {curve}, no table, c = {c}, sort {sort}")
        finally:
            bs.close()
    finally:
        gpu.lib().mnt753_msm_set_window_bits(old)


# ---- d. every bucket occupied ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,sort", [(8, "atomic"), (12, "atomic"), (12, "part"), (12, "generic")])
@pytest.mark.parametrize("curve", CURVES)
def test_every_bucket_occupied(gpu, curve, c, sort, monkeypatch):
    """dense(c) over 2^c bases in table mode: 1 .. 2^(c-1) put an entry into every bucket of the set, r - j fills the windows above; the
    reduction sees no empty bucket.  Small enough for the discrete logs and, at c = 8, the oracle."""
    monkeypatch.setenv("MNT753_MSM_PRECOMP", "1")
    monkeypatch.setenv("MNT753_MSM_TABLE_BITS", str(c))
    monkeypatch.setenv("MNT753_MSM_SORT", sort)
    ints = S.dense(curve, c)
    seed = 9500 + curve
    pts = points(gpu, curve, 1, seed, len(ints))
    sc = S.wire(curve, ints)
    want = expected(gpu, curve, 1, seed, S.label("dense", c), 0, ints)
    bs = gpu.BaseSet(curve, 1, pts)
    try:
        got = gpu.point_to_affine(curve, 1, bs.msm(sc))
        plan = gpu.msm_last_plan()
    finally:
        bs.close()
    assert plan["window_table"] and plan["window_bits"] == c, plan
    assert np.array_equal(got, want), f"curve {curve}, dense({c}), sort {sort}"
    if c == 8:
        assert np.array_equal(want, O.msm(curve, 1, pts, sc))


# ---- e. the lane-split G2 kernels -----------------------------------------------------------------------------------------------------------
G2_FAMILIES = ("single_bits/4", "edges", "extremes")


@pytest.mark.parametrize("curve", CURVES)
def test_g2_with_the_table_at_the_width_its_plan_picks(gpu, curve, monkeypatch):
    """G2 (two / three lanes per point) with a forced table at the width the plan picks for the set: table rows w * entry_stride +
    base_offset + i.  Extremes of that width, the edges and every fourth single bit; the first 200 pairs against the oracle as well."""
    monkeypatch.setenv("MNT753_MSM_PRECOMP", "1")
    pts = points(gpu, curve, 2)
    bs = gpu.BaseSet(curve, 2, pts)
    try:
        gpu.point_to_affine(curve, 2, bs.msm(S.wire(curve, [1])))
        plan = gpu.msm_last_plan()
        assert plan["window_table"], plan
        c = plan["window_bits"]
        fams, total = layout(curve, c, G2_FAMILIES)
        assert total <= len(pts)
        run_families(gpu, curve, 2, bs, fams, f"curve {curve}, G2, table, c = {c}")
        assert gpu.msm_last_plan()["window_bits"] == c
        sc = S.wire(curve, [s for _, _, ints in fams for s in ints][:200])
        assert np.array_equal(gpu.point_to_affine(curve, 2, bs.msm(sc)), O.msm(curve, 2, pts[:200], sc)), f"curve {curve}, G2, table, c = {c}, first 200"
    finally:
        bs.close()


@pytest.mark.parametrize("sort", ["atomic", "part"])
@pytest.mark.parametrize("curve", CURVES)
def test_g2_without_the_table(gpu, curve, sort, monkeypatch):
    """the same families at c = 13 with one bucket set per window (58 sets of 4096 buckets), under both sort stages"""
    c = 13
    monkeypatch.setenv("MNT753_MSM_PRECOMP", "0")
    monkeypatch.setenv("MNT753_MSM_SORT", sort)
    fams, total = layout(curve, c, G2_FAMILIES)
    old = gpu.lib().mnt753_msm_set_window_bits(c)
    try:
        bs = gpu.BaseSet(curve, 2, points(gpu, curve, 2)[:total])
        try:
            run_families(gpu, curve, 2, bs, fams, f"curve {curve}, G2, no table, c = {c}, sort {sort}")
            plan = gpu.msm_last_plan()
            assert not plan["window_table"] and plan["window_bits"] == c, plan
        finally:
            bs.close()
    finally:
        gpu.lib().mnt753_msm_set_window_bits(old)


# ---- f. the reference itself ----------------------------------------------------------------------------------------------------------------
def libff_msm(tmp_path, curve, group, pts, sc):
    """the affine result words of libff's multi_exp_with_mixed_addition<BDLO12> over the same pairs (oracle/_ref/ref_msm_bench)"""
    ref = O.need_ref("ref_msm_bench")             # missing = failure on a GPU box (tests/oracle_lib.py)
    path = tmp_path / "pairs.bin"
    with open(path, "wb") as f:
        pts.tofile(f); sc.tofile(f)
    r = subprocess.run([ref, str(path), str(len(sc)), ("MNT4753", "MNT6753")[curve], f"G{group}"], capture_output=True, text=True, timeout=600)
    os.remove(path)
    assert r.returncode == 0, r.stderr[-1000:]
    hx = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])["result_affine_hex"]
    return np.array([int(hx[16 * i:16 * i + 16], 16) for i in range(len(hx) // 16)], dtype=np.uint64)


@pytest.mark.parametrize("curve", CURVES)
def test_families_vs_libff_multi_exp(gpu, curve, tmp_path):
    """All G1 families of width 16 and dense(8) as ONE list of pairs through libff's own multi_exp_with_mixed_addition: the reference
    agrees with the discrete logs on these scalars, and so does the product on the whole list under its default plan."""
    fams, total = layout(curve, 16, G1_FAMILIES)
    dense = S.dense(curve, 8)
    ints = [s for _, _, f in fams for s in f] + dense
    pts = points(gpu, curve, 1)[:len(ints)]
    sc = S.wire(curve, ints)
    want = libff_msm(tmp_path, curve, 1, pts, sc)
    assert np.array_equal(want, expected(gpu, curve, 1, base_seed(curve, 1), "all(16)+dense(8)", 0, ints))
    bs = gpu.BaseSet(curve, 1, pts)
    try:
        assert np.array_equal(gpu.point_to_affine(curve, 1, bs.msm(sc)), want)
    finally:
        bs.close()
