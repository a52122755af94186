"""GPU: the rows of a base set's device array (plain bases and window table) have a stride of their own -- 256 bytes on the base
fields, x and y each on a 128-byte line (csrc/msm_kernels.hip.h, row_words / row_y_off); the lane-split G2 fields keep packed rows.
Every reader of those rows, at sizes that are no multiple of a wave and with the side paths that load y directly, against the known
answer through the discrete logs of the synthetic bases.  Bit-exact (integer work)."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

SIZES = [1000, 4097]        # neither a multiple of 64; 4097 is the smallest set that gets a window table by default
LEVELS = [(1, 0), (2, 0), (3, 0), (1, 2), (2, 2), (3, 2)]   # (regular, irregular) batched-affine levels forced
_CACHE = {}


def g1_case(gpu, curve, n):
    """(bases, scalars, expected affine sum) of a G1 set whose first level meets equal and opposite points: repeated bases under
    the same scalar (every window doubles), a base next to its negative under the same scalar and a repeated base under the
    negated scalar (both cancel), plus zero / one scalars and an identity base.  The expectation goes through the discrete logs of
    the UNCHANGED generator output: the scalars are moved onto the bases they really multiply.  Computed once per (curve, n)."""
    key = (curve, n)
    if key not in _CACHE:
        seed = 5100 + curve
        pts = gpu.synth_points(curve, 1, seed, n)
        sc = gpu.synth_scalars(curve, seed + 50, n)
        eq = sc.copy()                                     # the same sum over the generator's own bases
        one = gpu.api.mont_one(curve)
        sc[3] = 0; eq[3] = 0
        sc[4] = one; eq[4] = one
        for j in range(16, 32, 2):                         # P, P under s: 2 s on P
            pts[j + 1] = pts[j]; sc[j + 1] = sc[j]
            eq[j] = O.field_op(curve, 1, sc[j], sc[j]); eq[j + 1] = 0
        for j in range(40, 56, 2):                         # P, -P under s
            pts[j + 1] = pts[j]; pts[j + 1, 12:] = O.neg_fq(curve, pts[j, 12:]); sc[j + 1] = sc[j]
            eq[j] = 0; eq[j + 1] = 0
        for j in range(64, 80, 2):                         # P under s, P under -s
            pts[j + 1] = pts[j]; sc[j + 1] = O.field_op(curve, 5, sc[j])
            eq[j] = 0; eq[j + 1] = 0
        j = n - 2                                          # ... and at the end of the set: the last rows of every window
        pts[j + 1] = pts[j]; sc[j + 1] = sc[j]
        eq[j] = O.field_op(curve, 1, sc[j], sc[j]); eq[j + 1] = 0
        pts[7] = 0; eq[7] = 0                              # identity base
        want = gpu.point_to_affine(curve, 1, gpu.synth_expected_msm(curve, 1, seed, eq))
        _CACHE[key] = (pts, sc, eq, want, seed)
    return _CACHE[key]


def run(gpu, bs, curve, group, sc, **kw):
    return gpu.point_to_affine(curve, group, bs.msm(np.ascontiguousarray(sc), **kw))


@pytest.mark.parametrize("table", [1, 0])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("curve", [0, 1])
def test_first_level_reads_rows(gpu, curve, n, table, monkeypatch):
    """Level 1 of the batched-affine pass gathers its operands from the rows: of the window table (every window index, the last row
    W n - 1 included: the set ends in a repeated base) and of the plain bases.  Levels forced to 1, 2 and 3, with 0 and 2 irregular ones."""
    pts, sc, _, want, _ = g1_case(gpu, curve, n)
    monkeypatch.setenv("MNT753_MSM_PRECOMP", str(table))
    bs = gpu.BaseSet(curve, 1, pts)
    try:
        for levels, irr in LEVELS:
            monkeypatch.setenv("MNT753_MSM_PAIR", str(levels))
            monkeypatch.setenv("MNT753_MSM_IRR", str(irr))
            got = run(gpu, bs, curve, 1, sc)
            plan = gpu.msm_last_plan()
            assert plan["window_table"] == bool(table) and plan["pair_levels"] == levels and plan["irr_levels"] == irr, plan
            assert np.array_equal(got, want), (levels, irr)
    finally:
        bs.close()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("curve", [0, 1])
def test_accumulate_kernel_gathers_rows(gpu, curve, n, monkeypatch):
    """No levels, window table on: the accumulate kernel's own row gather."""
    pts, sc, _, want, _ = g1_case(gpu, curve, n)
    monkeypatch.setenv("MNT753_MSM_PRECOMP", "1")
    monkeypatch.setenv("MNT753_MSM_PAIR", "0")
    bs = gpu.BaseSet(curve, 1, pts)
    try:
        got = run(gpu, bs, curve, 1, sc)
        plan = gpu.msm_last_plan()
        assert plan["window_table"] and plan["pair_levels"] == 0, plan
        assert np.array_equal(got, want)
    finally:
        bs.close()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("curve", [0, 1])
def test_sub_range_of_plain_bases(gpu, curve, n, monkeypatch):
    """An MSM over bases[offset : offset + m] without a table: the array is entered at offset * (row stride).  Through the accumulate
    kernel alone and through two levels; the expectation has zero scalars on the bases in front of the range."""
    pts, sc, eq, _, seed = g1_case(gpu, curve, n)
    off, m = 9, n - 109                                    # the range holds every special pair of the set but the last one
    lead = np.zeros((off, 12), dtype=np.uint64)
    want = gpu.point_to_affine(curve, 1, gpu.synth_expected_msm(curve, 1, seed, np.concatenate([lead, eq[off:off + m]])))
    assert not np.array_equal(sc[off:off + m], eq[off:off + m])      # the special pairs lie inside the range
    monkeypatch.setenv("MNT753_MSM_PRECOMP", "0")
    bs = gpu.BaseSet(curve, 1, pts)
    try:
        for levels in (0, 2):
            monkeypatch.setenv("MNT753_MSM_PAIR", str(levels))
            got = run(gpu, bs, curve, 1, sc[off:off + m], base_offset=off)
            plan = gpu.msm_last_plan()
            assert not plan["window_table"] and plan["pair_levels"] == levels, plan
            assert np.array_equal(got, want), levels
    finally:
        bs.close()


@pytest.mark.parametrize("curve", [0, 1])
def test_g2_rows_keep_their_stride(gpu, curve, monkeypatch):
    """The lane-split fields (G2 of both curves) stay on packed rows: table and plain bases, levels and accumulate kernel, a
    sub-range, with a repeated base (doubling in level 1)."""
    n, seed = 1000, 5200 + curve
    pts = gpu.synth_points(curve, 2, seed, n)
    sc = gpu.synth_scalars(curve, seed + 50, n)
    eq = sc.copy()
    for j in (16, 500, n - 2):
        pts[j + 1] = pts[j]; sc[j + 1] = sc[j]
        eq[j] = O.field_op(curve, 1, sc[j], sc[j]); eq[j + 1] = 0
    want = gpu.point_to_affine(curve, 2, gpu.synth_expected_msm(curve, 2, seed, eq))
    off, m = 9, n - 30
    want_sub = gpu.point_to_affine(curve, 2, gpu.synth_expected_msm(curve, 2, seed, np.concatenate([np.zeros((off, 12), dtype=np.uint64), eq[off:off + m]])))
    for table in ("1", "0"):
        monkeypatch.setenv("MNT753_MSM_PRECOMP", table)
        bs = gpu.BaseSet(curve, 2, pts)
        try:
            for levels, irr in ((2, 0), (1, 2), (0, 0)):
                monkeypatch.setenv("MNT753_MSM_PAIR", str(levels))
                monkeypatch.setenv("MNT753_MSM_IRR", str(irr))
                assert np.array_equal(run(gpu, bs, curve, 2, sc), want), (table, levels, irr)
                assert gpu.msm_last_plan()["window_table"] == (table == "1")
            assert np.array_equal(run(gpu, bs, curve, 2, sc[off:off + m], base_offset=off), want_sub), table
        finally:
            bs.close()
