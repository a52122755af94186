"""GPU: end to end against the reference prover on parameter sets whose evaluation domain is a step or an extended radix-2 domain.

tests/golden/domains/hashes.json (tools/mint_domain_hashes.py) records, per seeded synthetic parameter set of
tools/synth_files.write_files_d, the sha256 of the proof the reference's `main <curve> compute` wrote.  The files are regenerated
here from the seed and `main_hip` must write the same bytes -- as a one-shot prover, with --repeat 2, and (one set) sharded over two
logical devices.  Sizes the reference proves through a domain this library does not build (MNT6753 d + 1 = 40: mixed-radix basic) or
cannot prove at all (MNT4753 d + 1 = 21: the domain has 24 elements) make main_hip fail and write nothing."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import domain_ref as D
import golden_io as G
import oracle_lib as O
import synth_files

pytestmark = pytest.mark.gpu
EXE = os.path.join(O.ROOT, "snark-challenge-prover-reference_amd", "main_hip")
TABLE = json.load(open(os.path.join(G.GOLDEN, "domains", "hashes.json")))
CURVE = {"MNT4753": 0, "MNT6753": 1}
PROOFS = ["MNT4753_24", "MNT4753_1152", "MNT4753_24576", "MNT6753_12", "MNT6753_9216", "MNT6753_65536"]


def sha256_file(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for blk in iter(lambda: f.read(1 << 24), b""):
            h.update(blk)
    return h.hexdigest()


def run(args, env=None):
    return subprocess.run([EXE] + args, capture_output=True, text=True, env=dict(os.environ, **(env or {})), timeout=600)


def test_the_minted_table_is_complete():
    assert sorted(TABLE["proofs"]) == sorted(PROOFS)
    for key, e in TABLE["proofs"].items():
        kind, m = D.select(CURVE[e["curve"]], e["d"] + 1)
        assert m == e["d"] + 1 and kind in (D.STEP, D.EXTENDED), key
        assert e["d"] + 1 >= 1 << 16 or e["piecewise_host_agrees"] is True, key
    # the rows of the selection model that were put to the reference binary
    out = TABLE["reference_outcome"]
    assert out["MNT6753_40"]["succeeded"] is True               # through the mixed-radix basic domain
    assert out["MNT6753_50000"]["succeeded"] is False           # the domain (extended, 2^16) is larger than the vectors
    assert out["MNT4753_21"]["succeeded"] is False              # the domain (step, 24) is larger than the vectors
    assert all(e["agrees_with_model"] for e in out.values())


@pytest.mark.parametrize("key", PROOFS)
def test_prove_matches_the_reference_hash(gpu, key, tmp_path):
    e = TABLE["proofs"][key]
    curve = CURVE[e["curve"]]
    params, inp, out = (str(tmp_path / k) for k in ("params", "input", "proof"))
    synth_files.write_files_d(gpu, curve, e["d"], params, inp, seed=e["seed"])
    assert sha256_file(params) == e["params_sha256"], "synthetic parameter file differs from the one the reference proved"
    assert sha256_file(inp) == e["input_sha256"], "synthetic input file differs from the one the reference proved"
    runs = [([], {}), (["--repeat", "2"], {})]
    if key == "MNT4753_24576":
        runs.append((["--gpus", "2"], {"MNT753_SHARE_DEVICE": "1"}))     # compute_H spread over the devices: chains on 0 and 1, the join on 0
    for flags, env in runs:
        r = run([e["curve"], "compute", params, inp, out] + flags, env)
        assert r.returncode == 0, r.stderr[-2000:]
        assert os.path.getsize(out) == e["output_bytes"]
        assert sha256_file(out) == e["output_sha256"], f"proof differs from the reference's ({key}, flags {flags})"
        os.remove(out)


@pytest.mark.parametrize("name,m_dom,needles", [("MNT6753", 40, ("mixed-radix", " 40 ")), ("MNT4753", 21, ("d + 1 = 21", "24 elements"))])
def test_unprovable_sizes_fail_and_write_nothing(gpu, name, m_dom, needles, tmp_path):
    params, inp, out = (str(tmp_path / k) for k in ("params", "input", "proof"))
    synth_files.write_files_d(gpu, CURVE[name], m_dom - 1, params, inp, seed=TABLE["seed"])
    for flags in ([], ["--repeat", "2"]):
        r = run([name, "compute", params, inp, out] + flags)
        assert r.returncode != 0
        for needle in needles:
            assert needle in r.stderr, r.stderr[-2000:]
        assert not os.path.exists(out)


def test_compute_r1cs_on_a_step_domain(gpu, tmp_path):
    """compute-r1cs on the d + 1 = 24 set: a seeded random constraint system with nc + num_inputs + 1 <= 24 gives the proof that
    `compute` gives on an input file whose ca / cb / cc were evaluated here, in Python integers."""
    name, curve, m_dom = "MNT4753", 0, 24
    r_mod = D.MODULUS[curve]
    rinv = pow(D.R, -1, r_mod)
    params, inp = str(tmp_path / "params"), str(tmp_path / "input")
    d, m = synth_files.write_files_d(gpu, curve, m_dom - 1, params, inp, seed=TABLE["seed"])
    raw = np.fromfile(inp, dtype=np.uint64).reshape(-1, 12)
    w, r_el = raw[:m + 1], raw[m + 1 + 3 * (d + 1):]
    assert r_el.shape == (1, 12)
    nc, num_inputs = 20, 2
    assert nc + num_inputs + 1 <= m_dom
    rng = np.random.default_rng(0x723163)
    wi = D.mont_ints(w)
    mats, evals = [], []
    for k in range(3):
        counts = rng.integers(0, 5, size=nc)
        rp = np.zeros(nc + 1, dtype=np.uint64); rp[1:] = np.cumsum(counts)
        nnz = int(rp[nc])
        col = rng.integers(0, m + 1, size=nnz).astype(np.uint32)
        cf = gpu.synth_scalars(curve, 900 + k, nnz)
        mats.append((rp, col, cf))
        ci = D.mont_ints(cf)
        rows = [sum(ci[t] * wi[int(col[t])] * rinv for t in range(int(rp[i]), int(rp[i + 1]))) % r_mod for i in range(nc)]
        evals.append(rows + [0] * (m_dom - nc))
    for i in range(num_inputs + 1):                       # the input-consistency rows of the A polynomial
        evals[0][nc + i] = wi[i]
    r1cs, witness, direct = (str(tmp_path / k) for k in ("r1cs", "witness", "input_direct"))
    with open(r1cs, "wb") as f:
        np.array([num_inputs, m, nc], dtype=np.uint64).tofile(f)
        for rp, col, cf in mats:
            rp.tofile(f); col.tofile(f); cf.tofile(f)
    with open(witness, "wb") as f:
        w.tofile(f); r_el.tofile(f)
    with open(direct, "wb") as f:
        w.tofile(f)
        for v in evals:
            D.ints_to_words(v).tofile(f)
        r_el.tofile(f)
    out1, out2 = str(tmp_path / "proof_r1cs"), str(tmp_path / "proof_direct")
    r = run([name, "compute-r1cs", params, r1cs, witness, out1])
    assert r.returncode == 0, r.stderr[-2000:]
    r = run([name, "compute", params, direct, out2])
    assert r.returncode == 0, r.stderr[-2000:]
    assert os.path.getsize(out1) == 768 and open(out1, "rb").read() == open(out2, "rb").read()
    # a system that does not fit the parameters' evaluation domain is still refused
    with open(r1cs, "wb") as f:
        np.array([num_inputs, m, m_dom], dtype=np.uint64).tofile(f)
        for rp, col, cf in mats:
            np.concatenate([rp, np.full(m_dom - nc, rp[nc], dtype=np.uint64)]).tofile(f); col.tofile(f); cf.tofile(f)
    r = run([name, "compute-r1cs", params, r1cs, witness, out1 + ".big"])
    assert r.returncode != 0 and "does not fit the parameters' evaluation domain" in r.stderr
