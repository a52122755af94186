"""GPU: input validation on the device (csrc/mnt753_validate.hip) through the C ABI and through main_hip, against the big-integer
model of tests/validate_ref.py (which tests/test_validate_cpu.py pins to the reference's own data).  All comparisons are exact:
(n_bad, first_bad, reason of first_bad) for every case, expected values computed by the model for the array that was checked.
None of these inputs provokes a fault: a malformed point is data, the kernels only compute on it."""
import filecmp
import os
import subprocess

import numpy as np
import pytest

import golden_io as G
import oracle_lib as O
import validate_ref as V
from test_validate_cpu import EXE, FIXTURES, FIXTURE_IDS, NAME, g16

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 1000, 65537)
N_MAX = max(SIZES)
GROUPS = [(0, 1), (0, 2), (1, 1), (1, 2)]


def edge_indices(n, seed, extra=3):
    """lane, wave and workgroup edges below n, and a few seeded random ones"""
    rng = np.random.default_rng(seed)
    idx = {i for i in (0, 63, 64, 255, 256, n - 1) if 0 <= i < n}
    idx |= {int(v) for v in rng.integers(0, n, size=extra)}
    return sorted(idx)


def fault_kinds(curve, group):
    deg = V.degree(curve, group)
    return [("plus1", k) for k in range(2 * deg)] + [("x_q", 0), ("x_max", 0), ("x_q_and_y_plus1", 0), ("zero", 0), ("y_zero", 0), ("negative", 0)]


def disturb(curve, group, pt, kind):
    """one point (u64 words, modified in place) made malformed -- or replaced by something else that is well formed: the identity in
    both of its encodings, and the point's negative (the check is the curve equation, not an integrity check of the file)"""
    cv, deg = V.CURVES[curve], V.degree(curve, group)
    what, k = kind
    if what == "plus1":                      # component k of x | y, one unit in its lowest word
        pt[12 * k] += np.uint64(1)
    elif what == "x_q":
        pt[:12] = V.to_words([cv.q])[0]
    elif what == "x_max":
        pt[:12] = V.to_words([(1 << 768) - 1])[0]
    elif what == "x_q_and_y_plus1":          # both faults at one index: non-canonical is reported, it comes first
        pt[:12] = V.to_words([cv.q])[0]
        pt[12 * deg] += np.uint64(1)
    elif what == "zero":
        pt[:] = 0
    elif what == "y_zero":
        pt[12 * deg:] = 0
    elif what == "negative":
        ys = V.ints(pt[12 * deg:])
        pt[12 * deg:] = V.to_words([(cv.q - y) % cv.q for y in ys]).reshape(-1)
    else:
        raise AssertionError(what)


@pytest.fixture(scope="module")
def synthetic(gpu):
    """per group: N_MAX multiples of the generator and the model's verdict on each (all well formed)"""
    out = {}
    for curve, group in GROUPS:
        pts = gpu.synth_points(curve, group, 0x76616c + 10 * curve + group, N_MAX)
        out[(curve, group)] = (pts, V.point_verdicts(curve, group, pts))
    return out


def both_ways(gpu, curve, group, pts):
    """the report for a host pointer and for a device pointer: one and the same"""
    host = gpu.check_points(curve, group, pts)
    buf = gpu.DeviceBuffer.from_numpy(pts)
    dev = gpu.check_points(curve, group, buf.ptr.value, on_device=True, n=pts.shape[0])
    buf.close()
    assert host == dev, (host, dev)
    return host


@pytest.mark.parametrize("curve,params,inp", FIXTURES, ids=FIXTURE_IDS)
def test_reference_files_are_well_formed(gpu, curve, params, inp):
    d, m, sets = V.params_sets(curve, params)
    for name, (group, _, n, pts) in sets.items():
        assert gpu.check_points(curve, group, pts) == (0, 0, 0), name
    vec = V.input_vectors(inp, d, m)
    for name, v in vec.items():
        assert gpu.check_scalars(curve, v) == (0, 0, 0), name
    bufs = [gpu.DeviceBuffer.from_numpy(vec[k]) for k in ("ca", "cb", "cc")]
    assert gpu.check_products(curve, bufs[0].ptr.value, bufs[1].ptr.value, bufs[2].ptr.value, d + 1) == (0, 0, 0)


@pytest.mark.parametrize("curve,group", GROUPS)
def test_synthetic_points_are_well_formed(gpu, synthetic, curve, group):
    pts, verdicts = synthetic[(curve, group)]
    assert V.report(verdicts) == (0, 0, 0)
    assert both_ways(gpu, curve, group, pts[:4096]) == (0, 0, 0)
    assert both_ways(gpu, curve, group, pts) == (0, 0, 0)
    assert gpu.check_points(curve, group, pts[:0], n=0) == (0, 0, 0)


@pytest.mark.parametrize("curve,group", GROUPS)
def test_planted_faults_every_kind_at_every_edge(gpu, synthetic, curve, group):
    base, base_v = synthetic[(curve, group)]
    kinds = fault_kinds(curve, group)
    seen = set()
    for n in SIZES:
        for shift in range(len(kinds) if n == 1 else 3):      # n = 1: every kind at index 0; else three assignments of kinds to edges
            pts, verdicts = base[:n].copy(), list(base_v[:n])
            for j, i in enumerate(edge_indices(n, seed=1000 * n + shift)):
                kind = kinds[shift] if n == 1 else kinds[(j + shift * 5 + n) % len(kinds)]
                disturb(curve, group, pts[i], kind)
                verdicts[i] = V.point_verdict(curve, group, pts[i])
                seen.add((kind[0], verdicts[i]))
            want = V.report(verdicts)
            print(f"curve {curve} group {group} n {n} shift {shift}: expected {want}")
            assert both_ways(gpu, curve, group, pts) == want, (n, shift)
    # the model called every kind what the issue says it is
    assert {("plus1", V.OFF_CURVE), ("x_q", V.NONCANONICAL), ("x_max", V.NONCANONICAL), ("x_q_and_y_plus1", V.NONCANONICAL), ("zero", V.OK),
            ("y_zero", V.OK), ("negative", V.OK)} <= seen, seen


@pytest.mark.parametrize("curve,group", GROUPS)
def test_single_fault_is_found_where_it_is(gpu, synthetic, curve, group):
    """one bad point and nothing else: first_bad is that index, for every edge, every component and both reasons"""
    base, base_v = synthetic[(curve, group)]
    deg = V.degree(curve, group)
    for n in (1000, N_MAX):
        for j, i in enumerate(edge_indices(n, seed=77 + n, extra=2)):
            for kind in (("plus1", j % (2 * deg)), ("x_max", 0)):
                pts = base[:n].copy()
                disturb(curve, group, pts[i], kind)
                want = (1, i, V.point_verdict(curve, group, pts[i]))
                assert want[2] == (V.OFF_CURVE if kind[0] == "plus1" else V.NONCANONICAL)
                assert gpu.check_points(curve, group, pts) == want, (n, i, kind)


@pytest.mark.parametrize("curve,group", GROUPS)
def test_report_does_not_depend_on_scheduling(gpu, synthetic, curve, group):
    """many bad points spread over the whole array, ten times: ten identical reports"""
    base, base_v = synthetic[(curve, group)]
    pts, verdicts = base.copy(), list(base_v)
    rng = np.random.default_rng(5)
    kinds = fault_kinds(curve, group)
    for i in sorted({int(v) for v in rng.integers(300, N_MAX, size=400)}):
        disturb(curve, group, pts[i], kinds[i % len(kinds)])
        verdicts[i] = V.point_verdict(curve, group, pts[i])
    want = V.report(verdicts)
    assert want[0] > 100
    buf = gpu.DeviceBuffer.from_numpy(pts)
    got = [gpu.check_points(curve, group, buf.ptr.value, on_device=True, n=N_MAX) for _ in range(10)]
    assert got == [want] * 10


def test_every_point_bad(gpu, synthetic):
    base, _ = synthetic[(0, 1)]
    pts = base.copy()
    pts[:, 12] += np.uint64(1)
    want = V.report(V.point_verdicts(0, 1, pts))
    assert want == (N_MAX, 0, V.OFF_CURVE)
    assert both_ways(gpu, 0, 1, pts) == want


@pytest.mark.parametrize("curve", [0, 1])
def test_scalars(gpu, curve):
    r = V.CURVES[curve].r
    good, bad = [0, 1, r - 1], [r, r + 1, (1 << 768) - 1]
    assert gpu.check_scalars(curve, V.to_words(good)) == (0, 0, 0)
    for v in bad:
        assert gpu.check_scalars(curve, V.to_words([v])) == (1, 0, V.NONCANONICAL)
    base = gpu.synth_scalars(curve, 91, N_MAX)
    for n in SIZES:
        for shift in range(3):
            sc = base[:n].copy()
            for j, i in enumerate(edge_indices(n, seed=31 * n + shift)):
                sc[i] = V.to_words([(good + bad)[(j + shift + n) % 6]])[0]
            want = V.report(V.scalar_verdicts(curve, sc))
            host = gpu.check_scalars(curve, sc)
            buf = gpu.DeviceBuffer.from_numpy(sc)
            assert host == gpu.check_scalars(curve, buf.ptr.value, on_device=True, n=n) == want, (n, shift)
    assert gpu.check_scalars(curve, base[:0], n=0) == (0, 0, 0)


@pytest.mark.parametrize("curve", [0, 1])
def test_products(gpu, curve):
    """n = 2^16 seeded rows with c = a b except where planted; every row bad; a non-canonical operand is reported as such"""
    r, n = V.CURVES[curve].r, 1 << 16
    a, b = gpu.synth_scalars(curve, 51, n), gpu.synth_scalars(curve, 52, n)
    ri = V.rinv(r)
    c_int = [x * y * ri % r for x, y in zip(V.ints(a), V.ints(b))]        # wire words of a b: (a R)(b R) / R
    c = V.to_words(c_int)
    da, db = gpu.DeviceBuffer.from_numpy(a), gpu.DeviceBuffer.from_numpy(b)
    def run(cc):
        dc = gpu.DeviceBuffer.from_numpy(cc)
        try:
            return gpu.check_products(curve, da.ptr.value, db.ptr.value, dc.ptr.value, n)
        finally:
            dc.close()
    assert V.report(V.product_verdicts(curve, a, b, c)) == (0, 0, 0)
    assert run(c) == (0, 0, 0)
    for shift in range(3):
        cc = c.copy()
        for i in edge_indices(n, seed=9 + shift, extra=5):
            cc[i] = V.to_words([(c_int[i] + 1 + shift) % r])[0]
        want = V.report(V.product_verdicts(curve, a, b, cc))
        assert want[2] == V.UNSATISFIED and run(cc) == want
    cc = V.to_words([(v + 1) % r for v in c_int])
    want = V.report(V.product_verdicts(curve, a, b, cc))
    assert want == (n, 0, V.UNSATISFIED) and run(cc) == want
    cc = c.copy(); cc[300] = V.to_words([r + 5])[0]; cc[70] = V.to_words([(c_int[70] + 1) % r])[0]
    want = V.report(V.product_verdicts(curve, a, b, cc))
    assert want == (2, 70, V.UNSATISFIED) and run(cc) == want
    cc[70] = c[70]
    assert run(cc) == (1, 300, V.NONCANONICAL)
    assert gpu.check_products(curve, da.ptr.value, db.ptr.value, da.ptr.value, 0) == (0, 0, 0)


@pytest.mark.parametrize("curve", [0, 1])
def test_witness_against_its_constraint_system(gpu, curve):
    """mnt753_r1cs_check on the reference's example system: its witness satisfies it; with one variable replaced, first_bad is the lowest
    constraint row whose a b - c becomes non-zero -- computed here from the oracle's evaluation and big-integer products"""
    num_inputs, m, nc, mats = gpu.read_r1cs_file(g16(curve, "r1cs.bin"))
    w = np.fromfile(g16(curve, "witness.bin"), dtype=np.uint64).reshape(-1, 12)[:m + 1].copy()
    cs = gpu.R1cs(curve, num_inputs, m, nc, mats)
    n = nc + num_inputs + 1
    dw = gpu.DeviceBuffer.from_numpy(w)
    assert cs.check(dw.ptr.value) == (0, 0, 0)
    other = gpu.synth_scalars(curve, 1234, 1)[0]
    for var in (num_inputs + 1, m, 1):                 # the first auxiliary variable, the last variable, the public input
        w2 = w.copy(); w2[var] = other
        a, b, c = O.r1cs_evaluate(curve, num_inputs, nc, mats, w2, n)
        want = V.report(V.product_verdicts(curve, a, b, c))
        print(f"curve {curve} variable {var}: expected {want}")
        assert want[0] > 0 and want[1] < nc and want[2] == V.UNSATISFIED
        dw = gpu.DeviceBuffer.from_numpy(w2)
        assert cs.check(dw.ptr.value) == want, var
        # the same through the evaluation and the row check, as compute-r1cs --validate runs them
        outs = [gpu.DeviceBuffer(96 * n) for _ in range(3)]
        cs.evaluate(dw.ptr.value, outs[0].ptr.value, outs[1].ptr.value, outs[2].ptr.value, n)
        assert gpu.check_products(curve, outs[0].ptr.value, outs[1].ptr.value, outs[2].ptr.value, n) == want
    cs.close()


# ---- the CLI -------------------------------------------------------------------------------------------------------------------------
def cli(args, env=None, stdin=None):
    return subprocess.run([EXE] + args, capture_output=True, text=True, timeout=600, env=dict(os.environ, **(env or {})), input=stdin)


def disturbed_params(curve, params, dst, set_name, index, word):
    """a copy of the parameter file with one word of one point of one set raised by one; -> the model's verdict on that point"""
    _, _, sets = V.params_sets(curve, params)
    group, off, n, pts = sets[set_name]
    raw = np.fromfile(params, dtype=np.uint64)
    at = off // 8 + pts.shape[1] * index + word
    raw[at] += np.uint64(1)
    raw.tofile(dst)
    pt = pts[index].copy(); pt[word] += np.uint64(1)
    return V.point_verdict(curve, group, pt)


@pytest.mark.parametrize("curve", [0, 1])
def test_cli_check(gpu, curve, tmp_path):
    params, inp, expected = G.e2e_paths(curve)
    d, m, sets = V.params_sets(curve, params)
    r = cli([NAME[curve], "check", params, inp])
    assert r.returncode == 0, r.stdout + r.stderr
    for name, (_, _, n, _) in sets.items():
        assert f"{name}: {n} points ok\n" in r.stdout
    for name, n in (("w", m + 1), ("ca", d + 1), ("cb", d + 1), ("cc", d + 1), ("r", 1)):
        assert f"{name}: {n} scalars ok\n" in r.stdout
    assert f"constraints: {d + 1} rows satisfied\n" in r.stdout
    # one word of the y of a point of H raised by one
    bad = str(tmp_path / "bad_params")
    idx = sets["H"][2] // 2
    assert disturbed_params(curve, params, bad, "H", idx, 12) == V.OFF_CURVE
    r = cli([NAME[curve], "check", bad])
    assert r.returncode == 3 and f"H: 1 bad, first at {idx}: off curve\n" in r.stdout and f"A: {m + 1} points ok\n" in r.stdout, r.stdout + r.stderr
    # several devices (logical devices sharing the one GPU): every device checks its slices, the index is the file's
    r4 = cli([NAME[curve], "check", bad, "--gpus", "4"], env={"MNT753_SHARE_DEVICE": "1"})
    assert r4.returncode == 3 and r4.stdout == r.stdout, r4.stdout + r4.stderr
    out = tmp_path / "proof.bin"
    r = cli([NAME[curve], "compute", bad, inp, str(out), "--validate"])
    assert r.returncode == 3 and f"H: 1 bad, first at {idx}: off curve" in r.stderr and not out.exists(), r.stdout + r.stderr
    if curve == 1:                            # one component of a B2 point (x.c2)
        assert disturbed_params(curve, params, bad, "B2", 3, 24) == V.OFF_CURVE
        r = cli([NAME[curve], "check", bad])
        assert r.returncode == 3 and "B2: 1 bad, first at 3: off curve\n" in r.stdout, r.stdout
    # validation does not disturb the proof
    for flags in ([], ["--gpus", "2"]):
        r = cli([NAME[curve], "compute", params, inp, str(out), "--validate"] + flags, env={"MNT753_SHARE_DEVICE": "1"})
        assert r.returncode == 0 and "validate params" in r.stdout, r.stdout + r.stderr
        assert filecmp.cmp(str(out), expected, shallow=False)
        out.unlink()
    # an input whose rows do not hold: cc[5] raised by one
    raw = np.fromfile(inp, dtype=np.uint64)
    raw[12 * (m + 1 + 2 * (d + 1) + 5)] += np.uint64(1)
    bad_in = str(tmp_path / "bad_input"); raw.tofile(bad_in)
    r = cli([NAME[curve], "check", params, bad_in])
    assert r.returncode == 3 and f"constraint 5 of {d + 1} is not satisfied" in r.stdout, r.stdout
    r = cli([NAME[curve], "compute", params, bad_in, str(out), "--validate"])
    assert r.returncode == 3 and "constraint 5 of" in r.stderr and not out.exists()
    # the resident prover: a bad job between two good ones -- both good ones are proved, the process says 3 at the end
    outs = [str(tmp_path / f"o{k}") for k in range(3)]
    feed = f"{bad_in} {outs[1]}\n{inp} {outs[2]}\n"
    r = cli([NAME[curve], "compute", params, inp, outs[0], "--serve", "--quiet", "--validate"], stdin=feed)
    lines = r.stdout.strip().splitlines()
    assert r.returncode == 3 and [l.split()[0] for l in lines] == ["failed", "proved"] and lines[0].startswith(f"failed {outs[1]}: constraint 5 of"), r.stdout + r.stderr
    assert filecmp.cmp(outs[0], expected, shallow=False) and filecmp.cmp(outs[2], expected, shallow=False) and not os.path.exists(outs[1])


@pytest.mark.parametrize("curve", [0, 1])
def test_cli_check_r1cs(gpu, curve, tmp_path):
    p, cs, wit = g16(curve, "params.bin"), g16(curve, "r1cs.bin"), g16(curve, "witness.bin")
    num_inputs, m, nc, mats = gpu.read_r1cs_file(cs)
    r = cli([NAME[curve], "check-r1cs", p, cs, wit])
    assert r.returncode == 0 and f"constraints: {nc} rows satisfied\n" in r.stdout, r.stdout + r.stderr
    plain, checked = str(tmp_path / "plain"), str(tmp_path / "checked")
    assert cli([NAME[curve], "compute-r1cs", p, cs, wit, plain]).returncode == 0
    r = cli([NAME[curve], "compute-r1cs", p, cs, wit, checked, "--validate"])
    assert r.returncode == 0 and filecmp.cmp(plain, checked, shallow=False), r.stdout + r.stderr
    # the last variable replaced by another field element
    raw = np.fromfile(wit, dtype=np.uint64).reshape(-1, 12).copy()
    raw[m] = gpu.synth_scalars(curve, 1234, 1)[0]
    bad = str(tmp_path / "bad_witness"); raw.tofile(bad)
    a, b, c = O.r1cs_evaluate(curve, num_inputs, nc, mats, raw[:m + 1], nc + num_inputs + 1)
    n_bad, first, reason = V.report(V.product_verdicts(curve, a, b, c))
    assert n_bad > 0 and reason == V.UNSATISFIED
    r = cli([NAME[curve], "check-r1cs", p, cs, bad])
    assert r.returncode == 3 and f"constraint {first} of {nc} is not satisfied ({n_bad} in all)" in r.stdout, r.stdout + r.stderr
    os.remove(checked)
    r = cli([NAME[curve], "compute-r1cs", p, cs, bad, checked, "--validate"])
    assert r.returncode == 3 and f"constraint {first} of" in r.stderr and not os.path.exists(checked), r.stdout + r.stderr
    # and the mistake this option exists for: without it the unsatisfied witness is proved and the process reports success
    assert cli([NAME[curve], "compute-r1cs", p, cs, bad, checked]).returncode == 0 and os.path.exists(checked)
    # complete --validate: the same bytes; a key file with a point off its curve is refused
    full, full_v = str(tmp_path / "full"), str(tmp_path / "full_v")
    args = [NAME[curve], "complete", g16(curve, "keys.bin"), wit, g16(curve, "challenge.bin")]
    assert cli(args + [full, "--s-seed", "9"]).returncode == 0
    assert cli(args + [full_v, "--s-seed", "9", "--validate"]).returncode == 0 and filecmp.cmp(full, full_v, shallow=False)
    keys = np.fromfile(g16(curve, "keys.bin"), dtype=np.uint64); keys[12] += np.uint64(1)
    bad_keys = str(tmp_path / "bad_keys"); keys.tofile(bad_keys)
    os.remove(full_v)
    r = cli([NAME[curve], "complete", bad_keys, wit, g16(curve, "challenge.bin"), full_v, "--validate"])
    assert r.returncode == 3 and "off curve" in r.stderr and not os.path.exists(full_v)


@pytest.mark.timeout(1500)
@pytest.mark.parametrize("curve,log2_d", [(0, 20), (1, 15)])
def test_full_size_files(gpu, curve, log2_d, tmp_path):
    """Once at BASELINE size, on the seeded files of tools/synth_files.py: the parameter file is well formed (every set is multiples
    of the generator, with the identities synth_files plants at the ends of A, B1, B2); one point of L disturbed at 2^(log2_d - 1) + 1
    is found there; and the INPUT file is refused -- its points and scalars are good, but ca, cb, cc are three independent uniform
    vectors, so a row holds with probability 1 / r: every one of the d + 1 rows is unsatisfied, from row 0 on.  That is the right
    verdict on these files (and why --validate cannot be a default while the benchmark proves them)."""
    import synth_files
    params, inp = str(tmp_path / "params"), str(tmp_path / "input")
    d, m = synth_files.write_files(gpu, curve, log2_d, params, inp)
    r = cli([NAME[curve], "check", params])
    assert r.returncode == 0, r.stdout + r.stderr
    for name, n in (("A", m + 1), ("B1", m + 1), ("B2", m + 1), ("L", m - 1), ("H", d)):
        assert f"{name}: {n} points ok\n" in r.stdout, r.stdout
    r = cli([NAME[curve], "check", params, inp])
    print(r.stdout)
    assert r.returncode == 3, r.stdout + r.stderr
    for name, n in (("A", m + 1), ("H", d)):
        assert f"{name}: {n} points ok\n" in r.stdout
    for name, n in (("w", m + 1), ("ca", d + 1), ("cb", d + 1), ("cc", d + 1), ("r", 1)):
        assert f"{name}: {n} scalars ok\n" in r.stdout, r.stdout
    assert f"constraint 0 of {d + 1} is not satisfied ({d + 1} in all)\n" in r.stdout, r.stdout
    # one word of L[idx].y raised by one, in place
    g1 = 24 * 8
    g2 = g1 * (2 if curve == 0 else 3)
    idx = (1 << (log2_d - 1)) + 1
    at = 16 + 2 * g1 * (m + 1) + g2 * (m + 1) + g1 * idx + 96
    with open(params, "r+b") as f:
        f.seek(16 + 2 * g1 * (m + 1) + g2 * (m + 1) + g1 * idx)
        pt = np.frombuffer(f.read(g1), dtype=np.uint64).copy()
        pt[12] += np.uint64(1)
        assert V.point_verdict(curve, 1, pt) == V.OFF_CURVE
        f.seek(at)
        f.write(pt[12:13].tobytes())
    r = cli([NAME[curve], "check", params])
    assert r.returncode == 3 and f"L: 1 bad, first at {idx}: off curve\n" in r.stdout and f"H: {d} points ok\n" in r.stdout, r.stdout + r.stderr
