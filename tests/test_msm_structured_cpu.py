"""CPU: the scalar families of tests/msm_structured.py do what they are built for -- the reference recoding reconstructs every one of
them at every width, the extreme digit +-2^(c-1) is reached in every window where a scalar below r can have it, every bit position
lands in a window -- and the two references tests/test_msm_structured_gpu.py rests on (the oracle's windowed multi-exp, which has
never seen such scalars either, and the discrete logs of the synthetic bases) agree on them."""
import numpy as np
import pytest

import msm_structured as S
import oracle_lib as O

CURVES = [0, 1]


def all_families(curve, c):
    return [(S.label(name, c), S.family(curve, name, c)) for name in ("single_bits", "extremes", "carry_chains", "edges")]


@pytest.mark.parametrize("c", S.WIDTHS)
@pytest.mark.parametrize("curve", CURVES)
def test_recoding_reconstructs_every_scalar(curve, c):
    """sum_w d_w 2^(wc) = s and |d_w| <= 2^(c-1), for every family (the dense one at the widths the GPU tests use it at)"""
    fams = all_families(curve, c)
    if c in (8, 12):
        fams.append((S.label("dense", c), S.dense(curve, c)))
    r, half, W = S.modulus(curve), 1 << (c - 1), S.windows(c)
    for name, ints in fams:
        assert ints and len(set(ints)) == len(ints), name
        for s in ints:
            assert 0 <= s < r, name
            d = S.booth(s, c)
            assert len(d) == W and S.unbooth(d, c) == s, (name, hex(s))
            assert max(d) <= half and min(d) >= -half, (name, hex(s))


@pytest.mark.parametrize("c", S.WIDTHS)
@pytest.mark.parametrize("curve", CURVES)
def test_extreme_digit_in_every_window_that_can_hold_it(curve, c):
    """extremes(c) and edges together give -2^(c-1) in every window 0 .. W-2 and +2^(c-1) in every window 1 .. W-2, and in the top
    window exactly what a scalar below r can give there.  The expected set is worked out, not read off the families:
      window 0 never holds +2^(c-1): there is no bit below it, and the window alone is at most 2^(c-1) - 1 before it turns negative;
      the top window never holds a negative digit: its top bit is bit W c - 1 >= 753, which no scalar has;
      the top window holds +2^(c-1) if and only if the largest digit it can have, the one of r - 1 (msm_structured.top_digit_max),
      is that large -- which at c = 2 it is (the window is r's top bit alone, plus a carry)."""
    half, W = 1 << (c - 1), S.windows(c)
    assert (W - 1) * c <= 753 <= W * c - 1     # the top window starts inside the scalar or right behind it (c | 753: carries only)
    want = {(w, -half) for w in range(W - 1)} | {(w, half) for w in range(1, W - 1)}
    top = S.top_digit_max(curve, c)
    assert 0 < top <= half
    if top == half:
        want.add((W - 1, half))
    cov = S.coverage(S.extremes(curve, c) + S.edges(curve), c)
    assert {(w, d) for w, d in cov if abs(d) == half} == want
    assert (W - 1, top) in cov                                     # r - 1 is one of the edges
    if c == 2:
        assert (W - 1, half) in want


@pytest.mark.parametrize("curve", CURVES)
def test_extremes_come_in_the_pairs_their_construction_promises(curve):
    """2^(wc+c-1): d_w = -2^(c-1), d_(w+1) = +1;  2^(wc+c-1) - 2^(wc-1): d_w = +2^(c-1), d_(w-1) = -2^(c-1); every other digit zero"""
    for c in S.WIDTHS:
        half, W = 1 << (c - 1), S.windows(c)
        members = set(S.extremes(curve, c))
        for w in range(W - 1):
            s = 1 << (w * c + c - 1)
            assert s in members
            assert S.booth(s, c) == [0] * w + [-half, 1] + [0] * (W - w - 2)
        for w in range(1, W - 1):
            s = (1 << (w * c + c - 1)) - (1 << (w * c - 1))
            assert s in members
            assert S.booth(s, c) == [0] * (w - 1) + [-half, half] + [0] * (W - w - 1)


@pytest.mark.parametrize("curve", CURVES)
def test_single_bits_reach_every_window_and_carry_chains_jump(curve):
    bits = S.single_bits(curve)
    assert bits == [1 << k for k in range(753)]
    for c in S.WIDTHS:
        W = S.windows(c)
        assert {w for w, _ in S.coverage(bits, c)} == set(range(W)), c
        # a top window that holds nothing but the carry (c divides 753): only bit 752 reaches it
        if (W - 1) * c == 753:
            assert S.booth(bits[752], c)[-2:] == [-(1 << (c - 1)), 1]
        for s in S.carry_chains(curve, c):
            d = S.booth(s, c)
            k = s.bit_length()
            assert d[0] == -1 and [x for x in d[1:] if x] == [1 << (k % c)] and d[k // c] == 1 << (k % c), (c, k)
    assert any((S.windows(c) - 1) * c == 753 for c in S.WIDTHS)       # c = 3


@pytest.mark.parametrize("c", [8, 12])
@pytest.mark.parametrize("curve", CURVES)
def test_dense_fills_every_bucket_of_window_zero(curve, c):
    half = 1 << (c - 1)
    zero = [S.booth(s, c)[0] for s in S.dense(curve, c)]
    assert zero[:half] == list(range(1, half)) + [-half]               # 2^(c-1) is the window's top bit: -2^(c-1), and +1 above
    assert zero[half:] == [-j for j in range(half)]
    assert {abs(d) for d in zero if d} == set(range(1, half + 1))      # every bucket of the set
    assert len({w for w, _ in S.coverage(S.dense(curve, c), c)}) > S.windows(c) // 2     # and the windows above are populated


def families_for_reference_agreement(curve):
    return [("extremes(16)", S.extremes(curve, 16)), ("carry_chains(16)", S.carry_chains(curve, 16)), ("dense(8)", S.dense(curve, 8))]


@pytest.mark.parametrize("curve", CURVES)
def test_oracle_and_discrete_logs_agree_on_the_families(pkg, curve):
    """G1, bases synth_points(curve, 1, seed, n): the oracle's O.msm (libff's BDLO12 restated, 16-bit chunks of its own) against
    (sum_k s_k e_k mod r) G through the known discrete logs e_k of the bases (synth_expected_msm).  Both run on the host: neither the
    product library nor the test library needs a device for this."""
    seed = 9300 + curve
    fams = families_for_reference_agreement(curve)
    pts = pkg.synth_points(curve, 1, seed, max(len(ints) for _, ints in fams), threads=2)
    for name, ints in fams:
        sc = S.wire(curve, ints)
        want = pkg.point_to_affine(curve, 1, pkg.synth_expected_msm(curve, 1, seed, sc))
        assert want.any(), name
        assert np.array_equal(O.msm(curve, 1, pts[:len(ints)], sc), want), name
        assert np.array_equal(O.msm(curve, 1, pts[:len(ints)], sc, chunks=3), want), name


def test_wire_is_the_montgomery_form_the_oracle_reads():
    """as_bigint (field_op 4) of the oracle gives the integers back"""
    import domain_ref as D
    for curve in CURVES:
        ints = S.edges(curve)
        for s, w in zip(ints, S.wire(curve, ints)):
            assert D.mont_ints(O.field_op(curve, 4, w))[0] == s
