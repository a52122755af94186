"""CPU: the designed constraint systems of tests/r1cs_designed.py -- their integer model against the oracle's restatement of the witness
map (oracle_r1cs_evaluate: r1cs_to_qap.tcc:223-237) on the full system and on every shape, the chunk-and-fold model of the column sums
against qap_ref.instance_map with the Lagrange values BY DEFINITION, and tools/host_r1cs_check.cpp: the kernels' lazy loops compiled for
the host with their bounds asserted, and its three mutants, each of which has to fail."""
import os
import subprocess

import numpy as np
import pytest

import domain_ref as D
import oracle_lib as O
import qap_ref as Q
import r1cs_designed as RD

ROOT = O.ROOT
CHUNK_TERMS = 256                                       # QAP_CHUNK_TERMS of csrc/qap_transpose.hpp; the GPU test reads it from the plan
SMALL = {0: (D.BASIC, 16), 1: (Q.MIXED, 20)}           # domains small enough for lagrange_def, for chunks of 4 terms
FULL = {0: (D.BASIC, 1024), 1: (Q.MIXED, 640)}         # the smallest domains that hold 2 L + 2 rows at L = 256


def random_t(curve, seed):
    return int.from_bytes(np.random.default_rng(seed).bytes(96), "little") % D.MODULUS[curve]


def oracle_equals_model(system, out_len):
    got = O.r1cs_evaluate(system.curve, system.num_inputs, system.nc, RD.matrices(system), RD.witness_words(system), out_len)
    for g, w in zip(got, RD.evaluate_words(system, out_len)):
        assert np.array_equal(g, w)


@pytest.mark.parametrize("curve", [0, 1])
def test_designed_elements_are_what_the_kernel_is_to_see(curve):
    r = D.MODULUS[curve]
    el = RD.elements(curve)
    words = D.to_wire(curve, el)
    assert D.mont_ints(words)[:11] == [x for _, x in RD.wire_targets(curve)]
    assert el[-3:] == [1, 2, r - 1] and len(el) == 14
    dev = lambda v: v * (1 << 756) % r                  # the device form modulo r
    c, x = RD.largest_pair(curve)
    assert dev(c) == r - 1 and x * D.R % r == r - 1
    assert dev(el[2]) < r >> 11                         # wire r - 1: a tiny device form


@pytest.mark.parametrize("curve", [0, 1])
def test_every_class_of_rows_is_present(curve):
    system, info = RD.designed_system(curve)
    r = D.MODULUS[curve]
    sums = RD.row_sums(system)
    assert system.nc < 1200 and sum(len(row) for row in system.rows[0]) > 1500
    assert sum(1 for s in sums[0] if s == 0) >= 40 and sums[0].count(1) >= 14 and sums[0].count(r - 1) >= 14
    lengths = {len(row) for row in system.rows[0]}
    assert lengths >= {0, 1, 2, 3, 4, 5, 8, 200, 201}
    for cls in ("zero2", "zero3", "zero8"):
        assert len(info[cls]) == 14
    for rows in system.rows:
        assert rows[0] == [] and rows[-1] == []
    assert sorted(map(str, system.rows[1])) == sorted(map(str, system.rows[0]))      # the same rows, in another order
    names = [n for n, _, _ in RD.shapes(curve)]
    assert set(names) >= {"nc0+0", "nc0+5", "nc1", "inputs0", "inputs_m", "exact", "zero_tail", "len255", "len256", "len257", "b_empty"}


@pytest.mark.parametrize("curve", [0, 1])
def test_model_equals_the_oracle_on_the_designed_system(curve):
    system, _ = RD.designed_system(curve)
    oracle_equals_model(system, system.nc + system.num_inputs + 1 + 9)


@pytest.mark.parametrize("curve", [0, 1])
def test_model_equals_the_oracle_on_every_shape(curve):
    for name, system, out_len in RD.shapes(curve):
        oracle_equals_model(system, out_len)
    sw = RD.swap_system(curve)
    n = sw.nc + sw.num_inputs + 1
    oracle_equals_model(sw, n)
    oracle_equals_model(RD.swapped(sw), n)
    a, b, _ = RD.evaluate(sw, n)
    a2, b2, _ = RD.evaluate(RD.swapped(sw), n)
    assert a2[:sw.nc] == b[:sw.nc] and b2[:sw.nc] == a[:sw.nc] and a2[sw.nc:] == a[sw.nc:]


@pytest.mark.parametrize("curve", [0, 1])
def test_satisfied_variant_and_its_disturbed_rows(curve):
    system, _, disturb = RD.satisfied_system(curve)
    r = D.MODULUS[curve]
    n = system.nc + system.num_inputs + 1
    oracle_equals_model(system, n)
    a, b, c = RD.evaluate(system, n)
    assert all(x * y % r == z for x, y, z in zip(a, b, c))
    a, b, c = RD.evaluate(RD.disturbed(system, disturb), n)
    assert [i for i in range(n) if a[i] * b[i] % r != c[i]] == sorted(disturb)


@pytest.mark.parametrize("curve", [0, 1])
def test_column_model_equals_the_instance_map_by_definition(curve):
    """chunks of 4 terms on a domain of 16 / 20 points, u from lagrange_def: the chunk-and-fold model against the reference's plain loop,
    and lagrange_fast (which the GPU test uses at 1024 / 640 points) against the definition"""
    kind, dm = SMALL[curve]
    L = 4
    t = random_t(curve, 90 + curve)
    u = Q.lagrange_def(curve, kind, dm, t)
    assert u == Q.lagrange_fast(curve, kind, dm, t)
    qs = RD.qap_system(curve, L, u)
    assert qs.nc + qs.num_inputs + 1 <= dm
    for variant in (qs, RD.qap_variant(qs, (0, 1, 2)), RD.qap_variant(qs, (1,))):
        want = Q.instance_map(curve, variant.num_inputs, variant.nc, variant.m, RD.matrices_int(variant), u, t, dm)
        got = RD.qap_model(variant, u, check_classes=variant is qs)
        assert list(want[:3]) == got
    full = RD.qap_model(qs, u)
    assert len(RD.zero_columns(qs)) == 17 and all(full[which][col] == 0 for which, col in RD.zero_columns(qs))
    none =RD.qap_model(RD.qap_variant(qs, (0, 1, 2)), u, check_classes=False)
    assert none[0][:qs.num_inputs + 1] == u[qs.nc:qs.nc + qs.num_inputs + 1] and not any(none[0][qs.num_inputs + 1:]) and not any(none[1] + none[2])


@pytest.mark.parametrize("curve", [0, 1])
def test_column_model_at_the_device_chunk_size(curve):
    """the systems the GPU test runs (L = 256): every designed class asserted by the model, which equals the instance map"""
    kind, dm = FULL[curve]
    t = random_t(curve, 92 + curve)
    u = Q.lagrange_fast(curve, kind, dm, t)
    qs = RD.qap_system(curve, CHUNK_TERMS, u)
    assert qs.nc == 2 * CHUNK_TERMS + 2 and qs.nc + qs.num_inputs + 1 <= dm
    want = Q.instance_map(curve, qs.num_inputs, qs.nc, qs.m, RD.matrices_int(qs), u, t, dm)
    assert list(want[:3]) == RD.qap_model(qs, u)
    assert len(RD.zero_columns(qs)) == 1 + 9 + 3 + 4


@pytest.mark.parametrize("curve", [0, 1])
def test_t_inside_the_domain_picks_one_row(curve):
    """u is the indicator vector of the matching index: At / Bt / Ct are the coefficients of that row, or the 1 of an input row"""
    kind, dm = SMALL[curve]
    qs = RD.qap_system(curve, 4)
    r = D.MODULUS[curve]
    for j in RD.inside_indices(qs, dm):
        t = D.element(curve, Q._dkind(kind), dm, j)
        u = Q.lagrange_fast(curve, kind, dm, t)
        assert u == RD.indicator(dm, j) == Q.lagrange_def(curve, kind, dm, t)
        want = Q.instance_map(curve, qs.num_inputs, qs.nc, qs.m, RD.matrices_int(qs), u, t, dm)
        assert list(want[:3]) == RD.row_coefficients(qs, j) == RD.qap_model(qs, u, check_classes=False)
        assert want[3] == [pow(t, i, r) for i in range(dm + 1)] and Q.vanishing(curve, kind, dm, t) == 0
    assert any(any(v) for v in RD.row_coefficients(qs, 0)) and RD.row_coefficients(qs, qs.nc + 1)[0][1] == 1


def build_host_check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("host_r1cs") / "host_r1cs_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tools", "host_r1cs_check.cpp")], check=True, timeout=600)
    return str(exe)


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    return build_host_check(tmp_path_factory)


def test_lazy_loops_compiled_for_the_host(host_check):
    """the term loop of k_r1cs_evaluate / k_qap_chunks and the loop of k_qap_fold on every pair of designed operands: bounds after every
    step, words against the eager composition, zero sums as zero words"""
    out = subprocess.run([host_check], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout + out.stderr
    print(out.stdout)
    assert out.stdout.count("maxima:") == 2


@pytest.mark.parametrize("mutant", [1, 2, 3])
def test_each_mutant_of_the_loop_is_noticed(host_check, mutant):
    """1: no final fp_canon, 2: no flush on an odd count, 3: fp_norm once per three terms.  1 and 2 give wrong words on the designed
    operands (1 on every sum = 0); 3 keeps the words and leaves the stated bounds, which is all that stands between it and a lost carry"""
    out = subprocess.run([host_check, "--mutant", str(mutant)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 1 and "ALL OK" not in out.stdout and "checks failed" in out.stdout, out.stdout + out.stderr
    tally = {}
    for line in out.stdout.splitlines():
        if " cases, " in line:
            name, rest = line[:24].strip(), line[24:].split()
            tally[name] = (int(rest[0]), int(rest[2]), int(rest[6]))
    assert len(tally) == 9
    if mutant == 1:
        assert tally["sums = 0"][1] == tally["sums = 0"][0] and tally["fold: sums = 0"][1] == tally["fold: sums = 0"][0]
    elif mutant == 2:
        assert tally["chains, odd length"][1] > 0 and tally["fold: seed and partials"][1] > 0
        assert tally["chains, even length"] [1:] == (0, 0)
    else:
        assert tally["chains, odd length"][2] > 0 and tally["chains, even length"][2] > 0 and tally["fold: chains"][2] > 0
