"""CPU: every claim tests/pairing_designed.py makes about its members, the families through the project's own tower and Miller loop
compiled for the host (tools/host_pairing_check.cpp in its case-file mode: the one-lane fields, plain and under ASan + UBSan) against
the Python-integer model word for word, the signs of the relations between Miller values that tests/test_pairing_designed_gpu.py uses
between the device's own outputs, and the test library's new symbol."""
import os
import subprocess

import numpy as np
import pytest

import designed_points as DP
import field_raw_ref as FR
import oracle_lib as O
import pairing_designed as D
import subgroup_ref as SG
from test_abi_cpu import header_symbols

ROOT = O.ROOT
CURVES = (0, 1)


# ---- claims -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_family_counts_and_lookups(curve):
    fam = D.families(curve)
    assert {k: len(v) for k, v in fam.items()} == D.COUNTS[curve]
    assert len(D.elements(curve)) == sum(D.COUNTS[curve][k] for k in ("edge", "subfield", "unitary"))
    assert len(D.miller_pairs(curve)) == D.MILLER_COUNTS[curve] <= D.MAX_PAIRS
    assert (D.MILLER_COUNTS[0], D.MILLER_COUNTS[1]) == (45, 48)
    assert D.member(curve, "subfield/-1").name == "subfield/-1" and D.miller_pair(curve, "gen/gen").name == "gen/gen"
    with pytest.raises(KeyError):
        D.member(curve, "edge/all/3")
    with pytest.raises(KeyError):
        D.miller_pair(curve, "gen/lifted9")
    with pytest.raises(KeyError):
        D.elements(curve, only=("edges",))
    with pytest.raises(KeyError):
        D.miller_index(curve, D.model(curve).C.gen(1), D.model(curve).C.mul(3, D.model(curve).C.gen(2), 2))
    with pytest.raises(ValueError):
        D.expected(curve, 5, D.member(curve, "edge/all/0").value)


@pytest.mark.parametrize("curve", CURVES)
def test_edge_members_hold_what_their_names_say(curve):
    P = D.model(curve)
    q, d = P.q, P.deg
    canon = dict(D.canonical_values(curve))
    assert canon["(q-1)/2"] * 2 % q == q - 1 and canon["(q+1)/2"] * 2 % q == 1
    stored = dict(D.stored_values(curve))
    targets = {name: target for name, space, target, _ in DP.edge_targets(curve) if space == "X"}
    for name, x in stored.items():
        assert 0 <= x < q and DP.stored(curve, x) % q == targets[name], name
    assert stored["X=one"] == 1
    assert all(v == FR.MASK for v in DP.stored_limbs(curve, stored["X=limbmax"])[:FR.NL - 1])     # limbs 0 .. 25
    assert DP.stored_limbs(curve, stored["X=2^28"])[:2] == [0, 1] and DP.stored_limbs(curve, stored["X=2^28-1"])[:2] == [FR.MASK, 0]
    for n, v in list(canon.items()) + list(stored.items()):
        assert D.flat(D.member(curve, f"edge/all/{n}").value) == [v] * (2 * d)
    seen = set()
    for n in D.SINGLE_VALUES:
        for pos in range(2 * d):
            comps = D.flat(D.member(curve, f"edge/one/{n}/c{pos // d}.c{pos % d}").value)
            assert comps[pos] == canon[n] and all(c not in canon.values() for i, c in enumerate(comps) if i != pos)
            seen.add((n, pos))
    assert len(seen) == 2 * 2 * d                                                                 # every component position


@pytest.mark.parametrize("curve", CURVES)
def test_subfield_and_unitary_members(curve):
    P = D.model(curve)
    C, d = P.C, P.deg
    nonzero = lambda x: not C.f_is_zero(x)
    f = D.member(curve, "subfield/F").value
    assert f[1] == P.f_zero and all(f[0])
    fq = D.member(curve, "subfield/Fq").value
    assert fq[1] == P.f_zero and fq[0][0] != 0 and not any(fq[0][1:])
    vf = D.member(curve, "subfield/vF").value
    assert vf[0] == P.f_zero and all(vf[1])
    assert P.sqr(D.member(curve, "subfield/-1").value) == P.one() and D.member(curve, "subfield/-1").value[0][0] == P.q - 1
    for m in D.families(curve)["unitary"]:
        assert D.norm(curve, m.value) == P.f_one, m.name                       # norm one over F: conj is the inverse
        assert P.mul(m.value, P.conj(m.value)) == P.one() and nonzero(m.value[1]), m.name
    # first-chunk values lie in the cyclotomic subgroup: their Phi_k(q)-th power is one
    for k in range(2):
        assert P.pow(D.member(curve, f"unitary/first_chunk/{k}").value, P.K["phi"]) == P.one()
    e = D.member(curve, "unitary/order_r/1").value
    assert e == D.generator_pairing(curve) and e != P.one() and P.pow(e, C.r) == P.one()          # r is prime: order exactly r
    assert D.member(curve, "unitary/order_r/2").value == P.sqr(e)
    assert P.mul(D.member(curve, "unitary/order_r/r-1").value, e) == P.one()


@pytest.mark.parametrize("curve", CURVES)
def test_operand_pairs_give_the_designed_results(curve):
    P = D.model(curve)
    zero = (P.f_zero, P.f_zero)
    kinds = {k: [] for k in D.PAIR_KINDS}
    for m in D.families(curve)["pairs"]:
        kinds[m.name.rsplit("/", 1)[1]].append(m)
    assert all(len(v) == 3 for v in kinds.values())
    for m in kinds["inverse"]:
        assert P.mul(m.a, m.b) == P.one()
    for m in kinds["conjugate"]:
        r = P.mul(m.a, m.b)
        assert r[1] == P.f_zero and r[0] == D.norm(curve, m.a)                 # c1 is exactly the zero words
    for m in kinds["negative"]:
        assert P.C.f_add(m.a[0], m.b[0]) == P.f_zero and P.C.f_add(m.a[1], m.b[1]) == P.f_zero
    assert all(m.b == P.one() for m in kinds["one"]) and all(m.b == zero for m in kinds["zero"])


@pytest.mark.parametrize("curve", CURVES)
def test_miller_pairs_are_on_their_curves_and_on_or_off_the_subgroup_as_named(curve):
    C = D.model(curve).C
    g1, g2 = C.gen(1), C.gen(2)
    prs = D.miller_pairs(curve)
    assert len({(m.P, m.Q) for m in prs}) == len(prs)
    for m in prs:
        assert m.P is not None and m.Q is not None and C.on_curve(m.P, 1) and C.on_curve(m.Q, 2), m.name
    edge = list(DP.edge_points(curve).values())
    sparse = [pt for _, pt in DP.sparse_points(curve)]
    assert len(edge) == 13
    for pt in edge:                                                            # each with G2::one() and with one sparse member
        partners = [m.Q for m in prs if m.P == pt and m.name.startswith("edge/")]
        assert len(partners) == 2 and partners[0] == g2 and partners[1] in sparse
    with_gen = {m.Q for m in prs if m.P == g1}
    off = SG.off_subgroup_points(curve)
    assert set(sparse) <= with_gen and all(set(off[k]) <= with_gen for k in ("lifted", "cofactor", "mixed"))
    assert {g2, C.neg(g2), C.add(g2, g2, 2)} <= with_gen
    inside = {g2: True, C.neg(g2): True, C.add(g2, g2, 2): True}
    for q in {m.Q for m in prs}:
        want = inside.get(q, False)                                            # sparse, lifted, cofactor, mixed: off the subgroup
        assert SG.in_subgroup(curve, q) == want, [m.name for m in prs if m.Q == q]
        assert D.stepping_never_meets_zero(curve, q)                           # the out-of-scope case does not occur
    for base, i, ip, iq in D.sign_table(curve):
        assert prs[ip].P == C.neg(prs[i].P) and prs[ip].Q == prs[i].Q and prs[iq].P == prs[i].P and prs[iq].Q == C.neg(prs[i].Q)
    assert len({i for row in D.sign_table(curve) for i in row[1:]}) == 7       # the generators in all four sign combinations, and x=0's three


# ---- the relations the GPU tests use between the device's own outputs, pinned in the model ------------------------------------------------
RELATION_SIGN, signed_conj = D.RELATION_SIGN, D.signed_conj


@pytest.mark.parametrize("curve", CURVES)
def test_relation_signs(curve):
    """On MNT6753 ML(P, -Q) = ML(-P, Q) = conj(ML(P, Q)); on MNT4753, whose loop count is negative (a closing step and an inversion),
    both are -conj(ML(P, Q)) -- so ML(P, -Q) != conj(ML(P, Q)) there.  -1 lies in the subfield the final exponentiation kills:
    e(-P, Q) = e(P, -Q) = e(P, Q)^-1 on both curves."""
    P = D.model(curve)
    ml, gt = D.miller_values(curve), D.pairing_values(curve)
    s = RELATION_SIGN[curve]
    for base, i, ip, iq in D.sign_table(curve):
        assert ml[ip] == signed_conj(curve, ml[i], s) and ml[ip] != signed_conj(curve, ml[i], -s), base
        assert ml[iq] == signed_conj(curve, ml[i], s) and ml[iq] != signed_conj(curve, ml[i], -s), base
        assert gt[ip] == gt[iq] == P.conj(gt[i]) and P.mul(gt[i], gt[ip]) == P.one(), base
    g = D.miller_index(curve, P.C.gen(1), P.C.gen(2))
    assert gt[g] == D.generator_pairing(curve)
    two = D.miller_index(curve, P.C.gen(1), P.C.add(P.C.gen(2), P.C.gen(2), 2))
    assert gt[two] == P.sqr(gt[g])                                             # bilinear on G2


# ---- the one-lane host build -----------------------------------------------------------------------------------------------------------------
def tower_cases(curve):
    """[(op, a values, b values, want values)] over the families"""
    P = D.model(curve)
    el = [m.value for m in D.elements(curve)]
    rev = list(reversed(el))
    prs = D.families(curve)["pairs"]
    cases = [(0, el, rev, [P.mul(x, y) for x, y in zip(el, rev)]),
             (0, [m.a for m in prs], [m.b for m in prs], [P.mul(m.a, m.b) for m in prs])]
    cases += [(op, el, el, [D.expected(curve, op, x) for x in el]) for op in [1, 2, 3] + list(range(11, 10 + P.k))]
    eu = [m.value for m in D.elements(curve, only=("edge", "unitary"))]
    cases.append((4, eu, eu, [D.expected(curve, 4, x) for x in eu]))
    nz = [x for x in el if not D.is_zero(curve, x)]
    assert len(nz) == len(el) - 1
    cases.append((5, nz, nz, [D.expected(curve, 5, x) for x in nz]))
    return cases


def write_case(path, curve, op, a_words, b_words):
    n = len(a_words)
    head = np.array([curve, op, n], dtype="<u8")
    path.write_bytes(head.tobytes() + np.asarray(a_words, dtype="<u8").tobytes() + np.asarray(b_words, dtype="<u8").tobytes())


@pytest.fixture(scope="module")
def case_files(tmp_path_factory):
    """[(curve, op, case file, expected words)]: written once, run through both programs"""
    d = tmp_path_factory.mktemp("pairing_cases")
    out = []
    for curve in CURVES:
        for k, (op, a, b, want) in enumerate(tower_cases(curve)):
            path = d / f"c{curve}_{k}_op{op}.bin"
            write_case(path, curve, op, D.words(curve, a), D.words(curve, b))
            out.append((curve, op, path, D.words(curve, want)))
        g1, g2 = D.miller_words(curve)
        path = d / f"c{curve}_miller.bin"
        write_case(path, curve, 20, g1, g2)
        out.append((curve, 20, path, D.words(curve, D.miller_values(curve))))
    return out


def run_case_files(exe, case_files, tmp_path):
    for curve, op, path, want in case_files:
        res = tmp_path / (path.name + ".out")
        r = subprocess.run([exe, "cases", str(path), str(res)], capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert r.returncode == 0 and "runtime error" not in r.stderr, (path.name, r.stdout + r.stderr)
        got = np.fromfile(res, dtype="<u8").astype(np.uint64).reshape(want.shape[0], -1)
        bad = [i for i in range(want.shape[0]) if not np.array_equal(got[i], want[i])]
        assert not bad, (curve, op, path.name, bad)


def test_families_through_the_host_build(case_files, tmp_path):
    """every family through Tower<F>, Ate<C>::final_exponentiation and Ate<C>::miller_loop over the one-lane fields: all words"""
    exe = tmp_path / "host_pairing_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tools", "host_pairing_check.cpp")], check=True, timeout=600)
    run_case_files(str(exe), case_files, tmp_path)
    r = subprocess.run([str(exe), "cases", str(case_files[0][2])], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 2 and "usage" in r.stdout                           # neither mode: refused, nothing run


def test_families_through_the_host_build_under_sanitizers(case_files, tmp_path):
    """the same case files through build/san/host_pairing_check_asan (-fsanitize=address,undefined): a stand-alone program, run directly"""
    r = subprocess.run(["make", "build/san/host_pairing_check_asan"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    run_case_files(os.path.join(ROOT, "build", "san", "host_pairing_check_asan"), case_files, tmp_path)


# ---- ABI ----------------------------------------------------------------------------------------------------------------------------------------
def test_the_new_hook_is_declared_and_exported(pkg):
    assert "mnt753_test_vk_set_gt" in header_symbols("mnt753_hip_test.h")
    assert hasattr(pkg.test_lib(), "mnt753_test_vk_set_gt")
    assert pkg.test_lib().mnt753_test_vk_set_gt(None, None) == -1              # bad argument, no device touched
    assert hasattr(pkg.VerificationKey, "test_set_gt")
