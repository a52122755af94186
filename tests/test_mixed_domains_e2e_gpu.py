"""GPU: end to end against the reference prover on MNT6753 parameter sets whose evaluation domain is a mixed-radix basic domain
(d + 1 = 2^a 5^b), which `main_hip` builds with --mixed-radix (or MNT753_MIXED_RADIX=1) and refuses without.

* d + 1 = 40: the proof the reference wrote is recorded in tests/golden/domains/hashes.json (reference_outcome.MNT6753_40);
* d + 1 = 50, 5 * 2^8, 25 * 2^9 and 5 * 2^15 = 163840 (beyond every radix-2 domain of MNT6753): tests/golden/domains/mixed_hashes.json,
  minted by tools/mint_mixed_hashes.py with the reference's `main <curve> compute`.
The files are regenerated here from the seed (tools/synth_files.write_files_d) and main_hip must write the same bytes.
* d + 1 = 2^15 + 2^14: candidate 7 selects 51200 elements, more than the vectors hold: no proof exists, nothing is written."""
import hashlib
import json
import os
import subprocess

import pytest

import domain_ref as D
import golden_io as G
import oracle_lib as O
import synth_files

pytestmark = pytest.mark.gpu
EXE = os.path.join(O.ROOT, "snark-challenge-prover-reference_amd", "main_hip")
OLD = json.load(open(os.path.join(G.GOLDEN, "domains", "hashes.json")))
TABLE = json.load(open(os.path.join(G.GOLDEN, "domains", "mixed_hashes.json")))
PROOFS = ["MNT6753_50", "MNT6753_1280", "MNT6753_12800", "MNT6753_163840"]


def sha256_file(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for blk in iter(lambda: f.read(1 << 24), b""):
            h.update(blk)
    return h.hexdigest()


def run(args, env=None):
    return subprocess.run([EXE] + args, capture_output=True, text=True, env=dict(os.environ, **(env or {})), timeout=600)


def files_of(gpu, e, tmp_path):
    params, inp, out = (str(tmp_path / k) for k in ("params", "input", "proof"))
    synth_files.write_files_d(gpu, 1, e["d"], params, inp, seed=e["seed"])
    assert sha256_file(params) == e["params_sha256"], "synthetic parameter file differs from the one the reference proved"
    assert sha256_file(inp) == e["input_sha256"], "synthetic input file differs from the one the reference proved"
    return params, inp, out


def test_the_minted_table_is_complete():
    assert sorted(TABLE["proofs"]) == sorted(PROOFS)
    for key, e in TABLE["proofs"].items():
        assert e["curve"] == "MNT6753" and D.select(1, e["d"] + 1) == (D.MIXED, e["d"] + 1), key
        assert e["d"] + 1 >= 1 << 16 or e["piecewise_host_agrees"] is True, key
    assert TABLE["proofs"]["MNT6753_163840"]["d"] + 1 == 5 << 15


def test_d_plus_1_40_gives_the_recorded_proof(gpu, tmp_path):
    e = OLD["reference_outcome"]["MNT6753_40"]
    assert e["succeeded"] is True and e["d"] == 39
    params, inp, out = files_of(gpu, e, tmp_path)
    for flags, env in ((["--mixed-radix"], {}), (["--mixed-radix", "--repeat", "2"], {}), ([], {"MNT753_MIXED_RADIX": "1"})):
        r = run(["MNT6753", "compute", params, inp, out] + flags, env)
        assert r.returncode == 0, r.stderr[-2000:]
        assert sha256_file(out) == e["output_sha256"], f"proof differs from the reference's (flags {flags}, env {env})"
        os.remove(out)
    # MNT753_MIXED_RADIX=0 is the default: the refusal
    r = run(["MNT6753", "compute", params, inp, out], {"MNT753_MIXED_RADIX": "0"})
    assert r.returncode != 0 and "mixed-radix" in r.stderr and not os.path.exists(out)


@pytest.mark.parametrize("key", PROOFS)
def test_prove_matches_the_reference_hash(gpu, key, tmp_path):
    e = TABLE["proofs"][key]
    params, inp, out = files_of(gpu, e, tmp_path)
    runs = [(["--mixed-radix"], {})]
    if key == "MNT6753_163840":
        runs.append((["--mixed-radix", "--gpus", "2"], {"MNT753_SHARE_DEVICE": "1"}))     # the chains on devices 0 and 1, the join on 0
    for flags, env in runs:
        r = run(["MNT6753", "compute", params, inp, out] + flags, env)
        assert r.returncode == 0, r.stderr[-2000:]
        assert os.path.getsize(out) == e["output_bytes"]
        assert sha256_file(out) == e["output_sha256"], f"proof differs from the reference's ({key}, flags {flags})"
        os.remove(out)


def test_candidate_7_larger_than_the_vectors(gpu, tmp_path):
    m_dom = (1 << 15) + (1 << 14)
    assert D.select(1, m_dom) == (D.MIXED, 51200)
    params, inp, out = (str(tmp_path / k) for k in ("params", "input", "proof"))
    synth_files.write_files_d(gpu, 1, m_dom - 1, params, inp, seed=TABLE["seed"])
    r = run(["MNT6753", "compute", params, inp, out, "--mixed-radix"])
    assert r.returncode != 0
    assert "51200 elements" in r.stderr and f"d + 1 = {m_dom}" in r.stderr, r.stderr[-2000:]
    assert not os.path.exists(out)
