"""GPU: the tower, the final exponentiation, the Miller loop and mnt753_pairing on the DESIGNED inputs of tests/pairing_designed.py, in
the one-lane and in the lane-split form, against the Python-integer model of tests/pairing_ref.py; and the accept / reject comparison of
the verifier on near misses: a key whose e(alpha, beta) differs from the true element in ONE bit, at every word position.  Every
comparison is of all words; there is no tolerance.

Lane placement: a launch holds 129 elements on MNT4753 and 86 on MNT6753 -- a workgroup of lane groups and a ragged tail -- the family
cycled; a second launch starts one wave of groups (32 / 21) further into the family, so every member meets other lane positions."""
import functools

import numpy as np
import pytest

import pairing_designed as D
import pairing_ref as PR

pytestmark = pytest.mark.gpu

CURVES = (0, 1)
SPLITS = (0, 1)


# ---- tower families ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def family(curve, which):
    """(names, values, words [count, gt_words]) of the element families named"""
    mem = D.elements(curve, only=which)
    return [m.name for m in mem], [m.value for m in mem], D.words(curve, [m.value for m in mem])


@functools.lru_cache(maxsize=None)
def expected_words(curve, which, op):
    """the model's answers over a family, computed once and shared by both forms and both launches (read-only)"""
    _, values, _ = family(curve, which)
    if op == 0:
        want = [D.expected(curve, 0, x, y) for x, y in zip(values, reversed(values))]
    else:
        want = [D.expected(curve, op, x) for x in values]
    w = D.words(curve, want)
    w.setflags(write=False)
    return w


ALL = ("edge", "subfield", "unitary")


@functools.lru_cache(maxsize=None)
def nonzero_family(curve):
    names, values, w = family(curve, ALL)
    keep = [i for i, v in enumerate(values) if not D.is_zero(curve, v)]
    assert len(keep) == len(values) - 1                       # zero is the only excluded input of the final exponentiation
    return [names[i] for i in keep], [values[i] for i in keep], w[keep]


def launches(curve, count):
    """the index sets of the two launches; on MNT6753 a designed member of its own sits in group 20 of a wave (lanes 60 to 62, beside
    the idle lane 63) and in group 0 of the next"""
    out = [D.placement(curve, count, rot) for rot in (0, 1)]
    assert all(len(idx) == D.LAUNCH[curve] and set(idx) == set(range(count)) for idx in out)
    if curve == 1:
        assert D.WAVE_GROUPS[1] == 21 and count > 21
        for idx in out:
            assert idx[20] != idx[21] and list(idx[:22]).count(idx[20]) == 1 and list(idx[:22]).count(idx[21]) == 1
        assert out[0][20] == 20 and out[0][21] == 21 and out[1][20] == 41 % count and out[1][21] == 42 % count
    return out


def run_family(gpu, curve, split, op, names, a_words, b_words, want):
    for idx in launches(curve, len(names)):
        got = gpu.api.test_tower_op(curve, split, op, a_words[idx], None if b_words is None else b_words[idx])
        bad = sorted({names[i] for k, i in enumerate(idx) if not np.array_equal(got[k], want[i])})
        assert not bad, (curve, split, op, bad)
    return got, idx


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("curve", CURVES)
def test_tower_operations_on_designed_elements(gpu, curve, split):
    """mul (each member with the member at the mirrored position), sqr, inv (0 -> 0), the unitary inverse and every Frobenius map on the
    edge, subfield and unitary families"""
    P = D.model(curve)
    names, values, w = family(curve, ALL)
    run_family(gpu, curve, split, 0, names, w, w[::-1].copy(), expected_words(curve, ALL, 0))
    for op in [1, 2, 3] + list(range(11, 10 + P.k)):
        run_family(gpu, curve, split, op, names, w, None, expected_words(curve, ALL, op))
    # the hook's 0 -> 0 of the inverse, on zero itself
    z = names.index("edge/all/0")
    assert D.is_zero(curve, values[z]) and not w[z].any()
    assert not gpu.api.test_tower_op(curve, split, 2, w[z:z + 1])[0].any()
    # on unitary members the inverse and the unitary inverse are the same words
    un, _, uw = family(curve, ("unitary",))
    assert np.array_equal(gpu.api.test_tower_op(curve, split, 2, uw), gpu.api.test_tower_op(curve, split, 3, uw)), un


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("curve", CURVES)
def test_designed_operand_pairs(gpu, curve, split):
    """(a, 1/a) -> 1, (a, conj a) -> the norm with c1 exactly the zero words, (a, -a), (a, 1), (a, 0), both operand orders"""
    P = D.model(curve)
    prs = D.families(curve)["pairs"]
    names = [m.name for m in prs]
    a, b = D.words(curve, [m.a for m in prs]), D.words(curve, [m.b for m in prs])
    want = D.words(curve, [P.mul(m.a, m.b) for m in prs])
    one = P.gt_to_words(P.one())
    half = a.shape[1] // 2
    for x, y in ((a, b), (b, a)):
        # not launches(): its "designed member in group 20 and in group 0 of the next wave" needs more than 21 members; these 15 cycle
        for idx in (D.placement(curve, len(names), rot) for rot in (0, 1)):
            got = gpu.api.test_tower_op(curve, split, 0, x[idx], y[idx])
            for k, i in enumerate(idx):
                assert np.array_equal(got[k], want[i]), (curve, split, names[i])
                if names[i].endswith("/inverse"):
                    assert np.array_equal(got[k], one), names[i]
                if names[i].endswith("/conjugate"):
                    assert not got[k, half:].any() and got[k, :half].any(), names[i]
                if names[i].endswith("/zero"):
                    assert not got[k].any(), names[i]
                if names[i].endswith("/one"):
                    assert np.array_equal(got[k], a[i]), names[i]


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("curve", CURVES)
def test_w0_power_on_edge_and_unitary_elements(gpu, curve, split):
    which = ("edge", "unitary")
    names, _, w = family(curve, which)
    run_family(gpu, curve, split, 4, names, w, None, expected_words(curve, which, 4))


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("curve", CURVES)
def test_final_exponentiation_of_every_nonzero_member(gpu, curve, split):
    """against the model on every member but zero; FE(1) = FE(-1) = 1; FE of every subfield member with c1 = 0 is 1 (the first chunk kills
    F); FE of an order-r element is the model's power of it"""
    P = D.model(curve)
    names, values, w = nonzero_family(curve)
    want = D.words(curve, [D.expected(curve, 5, v) for v in values])
    got, idx = run_family(gpu, curve, split, 5, names, w, None, want)
    one = P.gt_to_words(P.one())
    at = {names[i]: k for k, i in enumerate(idx)}
    assert np.array_equal(gpu.api.test_tower_op(curve, split, 5, one.reshape(1, -1))[0], one)          # FE(1) = 1
    for name in ("subfield/-1", "subfield/F", "subfield/Fq"):
        assert np.array_equal(got[at[name]], one), name
    for i, v in enumerate(values):
        if v[1] == P.f_zero:
            assert np.array_equal(got[at[names[i]]], one), names[i]
    # an element of order r: the final exponent (q^k - 1) / r taken modulo r, as a plain power in the model
    e = (P.q ** P.k - 1) // P.C.r % P.C.r
    for j in D.ORDER_R_POWERS:
        v = D.member(curve, f"unitary/order_r/{j}").value
        assert np.array_equal(got[at[f"unitary/order_r/{j}"]], P.gt_to_words(P.pow(v, e))), j


# ---- Miller pairs ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def miller_expected(curve):
    ml, gt = D.words(curve, D.miller_values(curve)), D.words(curve, D.pairing_values(curve))
    ml.setflags(write=False); gt.setflags(write=False)
    return ml, gt


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("curve", CURVES)
def test_unreduced_miller_value_of_designed_pairs(gpu, curve, split):
    """edge G1 points (x = 0, x = q - 1, stored residues at limb edges), sparse G2 points, twist points off the subgroup: against the
    model; and between the device's OWN outputs ML(-P, Q) = ML(P, -Q) = +-conj(ML(P, Q)), the sign pinned in the CPU suite, so that an
    error of the model cannot mask one of the device"""
    P = D.model(curve)
    names = [m.name for m in D.miller_pairs(curve)]
    g1, g2 = D.miller_words(curve)
    got = gpu.api.test_miller_loop(curve, split, g1, g2)
    want, _ = miller_expected(curve)
    bad = [names[i] for i in range(len(names)) if not np.array_equal(got[i], want[i])]
    assert not bad, (curve, split, bad)
    for base, i, ip, iq in D.sign_table(curve):
        rel = P.gt_to_words(D.signed_conj(curve, P.gt_from_words(got[i]), D.RELATION_SIGN[curve]))
        assert np.array_equal(got[ip], rel) and np.array_equal(got[iq], rel), (curve, split, base)
        assert not np.array_equal(got[ip], got[i])


@pytest.mark.parametrize("curve", CURVES)
def test_pairing_of_designed_pairs(gpu, curve):
    """mnt753_pairing on the same pairs in one batch, an identity pair between two designed pairs (and one at each end)"""
    P = D.model(curve)
    names = [m.name for m in D.miller_pairs(curve)]
    g1, g2 = D.miller_words(curve)
    _, want = miller_expected(curve)
    one = P.gt_to_words(P.one())
    n = len(names)
    slots = [0, 2, D.WAVE_GROUPS[curve], n + 3]              # where the identity pairs go
    a, b, w, label = [], [], [], []
    src = 0
    for pos in range(n + len(slots)):
        if pos in slots:
            k = slots.index(pos)
            a.append(np.zeros(24, dtype=np.uint64) if k % 2 == 0 else g1[0])
            b.append(g2[0] if k % 2 == 0 else np.zeros(g2.shape[1], dtype=np.uint64))
            w.append(one); label.append(f"identity{k}")
        else:
            a.append(g1[src]); b.append(g2[src]); w.append(want[src]); label.append(names[src])
            src += 1
    assert src == n
    got = gpu.pairing(curve, np.stack(a), np.stack(b))
    bad = [label[i] for i in range(len(label)) if not np.array_equal(got[i], w[i])]
    assert not bad, (curve, bad)


@pytest.mark.parametrize("curve", CURVES)
def test_designed_scalars_on_the_reduced_pairing(gpu, curve):
    """e([a] P, Q) = e(P, [a] Q) for a = 2 and a = r - 1, and e(P, Q) e(-P, Q) = 1 with the product taken on the device"""
    P = D.model(curve)
    C = P.C
    g1, g2 = C.gen(1), C.gen(2)
    w1 = lambda pt: np.array(C.affine_to_words(pt, 1), dtype=np.uint64)
    w2 = lambda pt: np.array(C.affine_to_words(pt, 2), dtype=np.uint64)
    ps, qs = [g1], [g2]
    for a in (2, C.r - 1):
        ps += [C.mul(a, g1, 1), g1]
        qs += [g2, C.mul(a, g2, 2)]
    assert ps[3] == C.neg(g1) and qs[4] == C.neg(g2)
    got = gpu.pairing(curve, np.stack([w1(p) for p in ps]), np.stack([w2(q) for q in qs]))
    e = P.gt_from_words(got[0])
    assert np.array_equal(got[0], P.gt_to_words(D.generator_pairing(curve)))
    assert np.array_equal(got[1], got[2]) and np.array_equal(got[1], P.gt_to_words(P.sqr(e)))
    assert np.array_equal(got[3], got[4]) and np.array_equal(got[3], P.gt_to_words(P.conj(e)))
    one = P.gt_to_words(P.one())
    for split in SPLITS:
        assert np.array_equal(gpu.api.test_tower_op(curve, split, 0, got[0:1], got[3:4])[0], one), split


# ---- near misses of the accept / reject comparison -------------------------------------------------------------------------------------------
PATHS = ("verify", "verify_subgroup", "verify_folded")


def accepts(vk, path, proof, inp):
    if path == "verify":
        v = list(vk.verify(proof, inp))
        assert v in ([0], [2]), v
        return v == [0]
    if path == "verify_subgroup":
        v = list(vk.verify(proof, inp, check_subgroup=True))
        assert v in ([0], [2]), v
        return v == [0]
    ok, status = vk.verify_folded(proof.reshape(1, -1), inp.reshape(1, -1), coefficients=[1])      # rho = 1: GT^rho is GT itself
    assert list(status) == [0]
    return ok


WORD_RANGES = (range(0, 8), range(8, 16), range(16, 24))
NEAR_MISS_CASES = [(c, p, h, k, t) for c in CURVES for p in PATHS for h in (0, 1) for k in range(2 + c) for t in range(len(WORD_RANGES))]


@pytest.mark.parametrize("curve,path,half,comp,third", NEAR_MISS_CASES)
def test_one_flipped_bit_of_the_keys_gt_rejects(gpu, curve, path, half, comp, third):
    """The fixture key accepts its proof; with e(alpha, beta) replaced (mnt753_test_vk_set_gt) by the true element with ONE bit flipped
    it must reject -- for every 32-bit word of the element (96 / 144), the flipped bit being bit (position mod 32), so it moves through
    the word.  k_groth16_verify compares word by word through group_all (`verify`, and with the subgroup test), k_fold_tail through
    f_equal (`verify_folded` with n = 1 and rho = 1).  A comparison that looks at one lane's component, at 23 of 24 words or at one half
    only fails here and nowhere else.  The flip can leave a component non-canonical (bits 17 .. 31 of its last word): k_fold_tail
    refuses such a key element outright, since loading it keeps 756 bits of a component -- before it had that check the positions 23
    and 95 (both curves) and 119 (MNT6753) were ACCEPTED on the folded path; they are the regression cases.  (Only this hook can store a
    non-canonical element: mnt753_vk_create stores what mnt753_pairing returned.  No product call was ever unsound.)
    Measured on the MI355X: a single-proof call takes 0.23 s (MNT4753) / 0.27 s (MNT6753) through `verify`, with or without the
    subgroup test, and 0.17 s / 0.22 s through `verify_folded`: one lane group works, the time is latency.  The 24 words of one
    component took 5.6 / 6.5 s and 4.1 / 5.2 s, so a case covers a third of them, 8 calls and the two accepting ones: 1.6 to 2.7 s."""
    alpha, beta, delta, abc, proof, inp = D.g16_fixture(curve)
    vk = gpu.VerificationKey(curve, alpha, beta, delta, abc)
    true = vk.gt().copy()
    assert np.array_equal(true, PR.vk_head(f"g16_mnt{4 if curve == 0 else 6}"))
    deg = 2 + curve
    try:
        assert accepts(vk, path, proof, inp)
        u32 = true.view(np.uint32)                                       # little-endian: the kernels' 32-bit word positions
        assert u32.size == 2 * 24 * deg
        missed = []
        for word in WORD_RANGES[third]:
            pos = (half * deg + comp) * 24 + word
            near = u32.copy()
            near[pos] ^= np.uint32(1 << (pos % 32))
            vk.test_set_gt(near.view(np.uint64))
            assert np.array_equal(vk.gt(), near.view(np.uint64)) and np.count_nonzero(vk.gt() != true) == 1
            if accepts(vk, path, proof, inp):
                missed.append(pos)
        vk.test_set_gt(true)
        assert np.array_equal(vk.gt(), true) and accepts(vk, path, proof, inp)
        assert not missed, (curve, path, missed)
    finally:
        vk.close()
