"""CPU: the key-generation fixtures tests/golden/keygen_mnt{4,6}_{full,cut21} (minted by the reference's own functions from given
randomness, tools/mint_keygen.sh) against the Python restatement tests/keygen_ref.py and the CPU oracle's group arithmetic -- every
scalar of a key is recomputed from r1cs_in.bin and randomness.bin, every point is scalar * generator -- and the file layouts of
GeneratedKey.write().  This pins fixture and model against each other before a GPU is involved."""
import hashlib
import os

import numpy as np
import pytest

import domain_ref as D
import keygen_ref as K
import oracle_lib as O

G1, G2 = 1, 2


def scale(curve, group, gen, scalars):
    """[s * gen for s in scalars] in the affine wire format, by the CPU oracle (a one-term multi-scalar multiplication each)"""
    return np.stack([O.msm(curve, group, gen, w) for w in D.to_wire(curve, scalars)])


def test_fixture_manifest():
    """tests/golden/keygen_SHA256SUMS lists every file of the four fixtures with its digest"""
    listed = {}
    for line in open(os.path.join(K.GOLDEN, "keygen_SHA256SUMS")):
        digest, name = line.split()
        listed[name] = digest
    on_disk = sorted(f"{os.path.basename(K.fixture_dir(c, t))}/{n}" for c, t in K.FIXTURES for n in os.listdir(K.fixture_dir(c, t)))
    assert sorted(listed) == on_disk and len(on_disk) == 4 * 10
    for name, digest in listed.items():
        assert hashlib.sha256(open(os.path.join(K.GOLDEN, name), "rb").read()).hexdigest() == digest, name


@pytest.fixture(scope="module")
def models():
    """per fixture: the index, the randomness, and key_scalars of r1cs_in.bin -- computed once, shared by the tests below"""
    out = {}
    for curve, tag in K.FIXTURES:
        d = K.fixture_dir(curve, tag)
        idx = K.index(curve, tag)
        ni, m, nc, mats = K.read_r1cs(os.path.join(d, "r1cs_in.bin"))
        t, alpha, beta, delta, g1 = K.randomness(curve, tag)
        ti, ai, bi, di = (D.from_wire(curve, x)[0] for x in (t, alpha, beta, delta))
        imats = [(rp, col, D.from_wire(curve, cf)) for rp, col, cf in mats]
        s = K.key_scalars(curve, ni, m, nc, imats, K.CLASS_KIND[idx["reference_class"]], idx["domain_size"], ti, ai, bi, di)
        out[(curve, tag)] = dict(dir=d, index=idx, ni=ni, m=m, nc=nc, mats=mats, g1=g1, scalars=s, alpha=ai, beta=bi, delta=di)
    return out


@pytest.mark.parametrize("fixture", K.FIXTURES, ids=K.fixture_id)
def test_fixture_properties(models, fixture):
    """what the fixtures were chosen for: the swap decision, the domain, the densities, the variables no matrix touches"""
    mo = models[fixture]
    idx, s = mo["index"], mo["scalars"]
    assert (mo["ni"], mo["m"]) == (1, 32) and mo["nc"] == (30 if fixture[1] == "full" else 21)
    a, b = K.touched(mo["m"], mo["mats"][0]), K.touched(mo["m"], mo["mats"][1])
    assert (a, b) == (idx["touched_a"], idx["touched_b"]) == ((32, 31) if fixture[1] == "full" else (11, 22))
    assert s["swapped"] == idx["swapped"] == (fixture[1] == "cut21")
    assert (idx["reference_class"], idx["domain_size"]) == (("basic_radix2_domain", 32) if fixture[1] == "full" else ("step_radix2_domain", 24))
    assert (s["non_zero_At"], s["non_zero_Bt"]) == (idx["non_zero_At"], idx["non_zero_Bt"])
    assert idx["untouched_variables"] == (0 if fixture[1] == "full" else 9)
    assert s["Zt"] != 0
    # r1cs.bin is r1cs_in.bin with a and b exchanged where the swap fired
    ni, m, nc, post = K.read_r1cs(os.path.join(mo["dir"], "r1cs.bin"))
    want = [mo["mats"][1], mo["mats"][0], mo["mats"][2]] if s["swapped"] else mo["mats"]
    assert (ni, m, nc) == (mo["ni"], mo["m"], mo["nc"])
    for (rp, col, cf), (wrp, wcol, wcf) in zip(post, want):
        assert np.array_equal(rp, wrp) and np.array_equal(col, wcol) and np.array_equal(cf, wcf)
    # input.bin: w | ca | cb | cc over the whole domain | r, w and r those of witness.bin
    inp = np.fromfile(os.path.join(mo["dir"], "input.bin"), dtype="<u8").reshape(-1, 12)
    wit = np.fromfile(os.path.join(mo["dir"], "witness.bin"), dtype="<u8").reshape(-1, 12)
    assert inp.shape[0] == m + 1 + 3 * idx["domain_size"] + 1 and wit.shape[0] == m + 2
    assert np.array_equal(inp[:m + 1], wit[:m + 1]) and np.array_equal(inp[-1], wit[-1])
    assert os.path.getsize(os.path.join(mo["dir"], "vk.txt")) > 0


@pytest.mark.parametrize("fixture", K.FIXTURES, ids=K.fixture_id)
def test_every_point_of_the_fixture_is_scalar_times_generator(pkg, models, fixture):
    curve = fixture[0]
    mo = models[fixture]
    s, g1 = mo["scalars"], mo["g1"]
    g2 = pkg.group_generator(curve, G2)
    assert np.array_equal(pkg.point_to_affine(curve, G1, pkg.point_scale(curve, G1, D.to_wire(curve, [mo["index"]["g1_multiple"]])[0],
                                                                     pkg.point_from_affine(curve, G1, pkg.group_generator(curve, G1)))), g1)
    d, m, q = K.split_params(curve, open(os.path.join(mo["dir"], "params.bin"), "rb").read(), mo["ni"])
    assert (d, m) == (mo["index"]["domain_size"] - 1, mo["m"])
    assert np.array_equal(q["A"], scale(curve, G1, g1, s["A"]))
    assert np.array_equal(q["B1"], scale(curve, G1, g1, s["B"]))
    assert np.array_equal(q["B2"], scale(curve, G2, g2, s["B"]))
    assert np.array_equal(q["L"], scale(curve, G1, g1, s["L"]))
    assert np.array_equal(q["H"], scale(curve, G1, g1, s["H"]))
    # zero scalars are identities, written as all-zero words; the cut system leaves 9 variables untouched
    for name, sc in (("A", s["A"]), ("B1", s["B"]), ("B2", s["B"]), ("L", s["L"])):
        zero = [i for i, v in enumerate(sc) if v == 0]
        assert len(zero) >= mo["index"]["untouched_variables"]
        assert all(not q[name][i].any() for i in zero) and all(q[name][i].any() for i in range(len(sc)) if i not in zero)
    w1, w2 = K.aff_words(curve, G1), K.aff_words(curve, G2)
    keys = np.fromfile(os.path.join(mo["dir"], "keys.bin"), dtype="<u8").astype(np.uint64)
    a1, b1, d1 = scale(curve, G1, g1, [mo["alpha"], mo["beta"], mo["delta"]])
    b2, d2 = scale(curve, G2, g2, [mo["beta"], mo["delta"]])
    assert np.array_equal(keys, np.concatenate([a1, b1, b2, d1, d2]))
    vk = np.fromfile(os.path.join(mo["dir"], "vk_elements.bin"), dtype="<u8").astype(np.uint64)
    assert np.array_equal(vk, np.concatenate([a1, b2, d2, scale(curve, G1, g1, s["ABC"]).reshape(-1)]))
    assert keys.size == 3 * w1 + 2 * w2 and vk.size == w1 + 2 * w2 + (mo["ni"] + 1) * w1


@pytest.mark.parametrize("fixture", K.FIXTURES, ids=K.fixture_id)
def test_written_files_have_the_fixture_layout(pkg, models, fixture, tmp_path):
    """GeneratedKey.write() on the fixture's own points (no device): params.bin with its two header words, keys.bin, vk_elements.bin
    and r1cs.bin come out byte for byte"""
    curve = fixture[0]
    mo = models[fixture]
    d, m, q = K.split_params(curve, open(os.path.join(mo["dir"], "params.bin"), "rb").read(), mo["ni"])
    w1, w2 = K.aff_words(curve, G1), K.aff_words(curve, G2)
    keys = np.fromfile(os.path.join(mo["dir"], "keys.bin"), dtype="<u8").astype(np.uint64)
    cuts = np.cumsum([0, w1, w1, w2, w1, w2])
    singles = {k: keys[cuts[i]:cuts[i + 1]] for i, k in enumerate(("alpha_g1", "beta_g1", "beta_g2", "delta_g1", "delta_g2"))}
    vk = np.fromfile(os.path.join(mo["dir"], "vk_elements.bin"), dtype="<u8").astype(np.uint64)
    q["ABC"] = vk[w1 + 2 * w2:]
    _, _, _, post = K.read_r1cs(os.path.join(mo["dir"], "r1cs.bin"))
    key = pkg.GeneratedKey.from_host(curve, mo["ni"], m, mo["nc"], d + 1, q, singles, post)
    assert key.counts == {"A": m + 1, "B1": m + 1, "B2": m + 1, "L": m - mo["ni"], "H": d, "ABC": mo["ni"] + 1}
    key.write(str(tmp_path))
    for name in K.QUERY_FILES:
        assert (tmp_path / name).read_bytes() == open(os.path.join(mo["dir"], name), "rb").read(), name
    head = np.frombuffer((tmp_path / "params.bin").read_bytes()[:16], dtype="<u8")
    assert head.tolist() == [mo["index"]["domain_size"] - 1, m]
    assert (tmp_path / "params.bin").stat().st_size == 16 + 8 * (w1 * (2 * (m + 1) + m - mo["ni"] + d) + w2 * (m + 1))


def test_model_on_a_small_hand_system():
    """the restatement on numbers small enough to check by eye: the swap needs STRICTLY more, c_i changes behind num_inputs, H has
    m_d - 1 entries"""
    r = D.MODULUS[0]
    a = (np.array([0, 2], dtype=np.uint64), np.array([1, 2], dtype=np.uint32), None)
    b = (np.array([0, 2], dtype=np.uint64), np.array([2, 2], dtype=np.uint32), None)
    assert K.touched(3, a) == 2 and K.touched(3, b) == 1
    assert K.swap_rule(3, [a, b, a])[0] is False and K.swap_rule(3, [b, a, a])[0] is True and K.swap_rule(3, [a, a, b])[0] is False
    got = K.combine(0, [1, 2, 3], [4, 5, 6], [7, 8, r - 1], 1, 10, 100, 1000)
    assert got == [100 * 1 + 10 * 4 + 7, 100 * 2 + 10 * 5 + 8, (100 * 3 + 10 * 6 - 1) * 1000 % r]
    assert K.h_scalars(0, 3, 4, 5, 7) == [35, 105, 315]
