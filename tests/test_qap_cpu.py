"""The QAP at a point without a GPU: the Python model (tests/qap_ref.py) against the reference-minted fixture (tests/golden/qap,
tools/mint_qap.sh), the declarations and exports of the new entry points, and the host builder of the column-major view
(csrc/qap_transpose.hpp) through tools/host_qap_check.cpp, compiled plain and under ASan + UBSan and run directly."""
import os
import re
import subprocess

import numpy as np
import pytest

import domain_ref as D
import qap_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INDEX = Q.index()
NEW_SYMBOLS = ["mnt753_domain_vanishing_at", "mnt753_domain_lagrange_at", "mnt753_vec_powers", "mnt753_r1cs_qap_at", "mnt753_r1cs_qap_plan"]


def _id(e):
    return f"mnt{4 if e['curve'] == 0 else 6}-{e['kind']}-{e['m']}"


def test_fixture_covers_the_kinds_and_sizes():
    """what the reference chose is what the sizes were picked for: basic 2, 8, 1024 and step 24, 1152 on both curves, mixed 40 and
    200 and extended 2^16 on MNT6753; every entry has the generic t, 0, and five domain elements"""
    got = {(e["curve"], e["kind"], e["m"]) for e in INDEX["lagrange"]}
    want = {(c, k, m) for c in (0, 1) for k, m in ((D.BASIC, 2), (D.BASIC, 8), (D.BASIC, 1024), (D.STEP, 24), (D.STEP, 1152))}
    want |= {(1, D.MIXED, 40), (1, D.MIXED, 200), (1, D.EXTENDED, 1 << 16)}
    assert got == want
    for e in INDEX["lagrange"]:
        assert e["m"] == e["min_size"] and e["t"][:2] == ["generic", "zero"] and len(e["t"]) == 7
        m = e["m"]
        assert e["t"][2:] == [f"element:{i}" for i in (0, 1, m // 2 - 1, m // 2, m - 1)]


@pytest.mark.parametrize("entry", INDEX["lagrange"], ids=_id)
def test_model_equals_the_reference(entry):
    """lagrange (by definition up to 64 elements, the closed forms above) and vanishing equal every record: in full below 2^16, by
    sha256 and on the sample at 2^16; the element records are the domain elements of domain_ref"""
    curve, kind, m = entry["curve"], entry["kind"], entry["m"]
    for label, t_w, zt_w, u_w, idx, sha in Q.lagrange_records(entry):
        t = D.from_wire(curve, t_w)[0]
        if label.startswith("element:"):
            assert t == D.element(curve, Q._dkind(kind), m, int(label.split(":")[1])), label
        elif label == "zero":
            assert t == 0
        assert D.to_wire(curve, [Q.vanishing(curve, kind, m, t)])[0].tolist() == zt_w.tolist(), label
        u = D.to_wire(curve, Q.lagrange(curve, kind, m, t))
        assert Q.sha256_words(u) == sha, label
        assert np.array_equal(u if idx is None else u[idx], u_w), label


@pytest.mark.parametrize("curve,kind,m", [(0, D.BASIC, 2), (1, D.BASIC, 8), (0, D.STEP, 24), (1, D.STEP, 24), (1, D.MIXED, 40)])
def test_closed_forms_equal_the_definition(curve, kind, m):
    """lagrange_fast against lagrange_def at 2, 8, 24, 40: a generic t, 0, and an element of either half"""
    r = D.MODULUS[curve]
    ts = [pow(3, 1000003, r), 0, D.element(curve, Q._dkind(kind), m, 1), D.element(curve, Q._dkind(kind), m, m - 1)]
    for t in ts:
        assert Q.lagrange_fast(curve, kind, m, t) == Q.lagrange_def(curve, kind, m, t)


@pytest.mark.parametrize("entry", INDEX["qap"], ids=lambda e: f"mnt{4 if e['curve'] == 0 else 6}")
def test_model_instance_map_equals_the_reference(pkg, entry):
    curve = entry["curve"]
    num_inputs, nv, nc, mats = pkg.read_r1cs_file(os.path.join(ROOT, "tests", "golden", entry["r1cs"]))
    assert (num_inputs, nv, nc) == (entry["num_inputs"], entry["num_variables"], entry["num_constraints"])
    t_w, at, bt, ct, ht, zt = Q.qap_record(entry)
    t = D.from_wire(curve, t_w)[0]
    kind, dm = D.select(curve, nc + num_inputs + 1)
    assert dm == entry["m"] and kind == D.BASIC
    u = Q.lagrange(curve, kind, dm, t)
    imats = [(rp, col, D.from_wire(curve, cf)) for rp, col, cf in mats]
    got = Q.instance_map(curve, num_inputs, nc, nv, imats, u, t, dm)
    for g, want in zip(got, (at, bt, ct, ht)):
        assert np.array_equal(D.to_wire(curve, g), want)
    assert D.to_wire(curve, [Q.vanishing(curve, kind, dm, t)])[0].tolist() == zt.tolist()


def test_entry_points_declared_and_exported(pkg):
    header = open(os.path.join(ROOT, "include", "mnt753_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (\w+)", out))
    L = pkg.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in exported, name
        assert getattr(L, name).argtypes is not None, name
    for name in ("vec_powers", "QapPlan"):
        assert hasattr(pkg, name)
    for cls, names in ((pkg.Domain, ("vanishing_at", "lagrange_at")), (pkg.R1cs, ("qap_at", "qap_plan"))):
        for n in names:
            assert callable(getattr(cls, n))


def test_refusals_come_before_the_device(pkg):
    """null pointers are MNT753_EINVAL with a message whether or not a device exists"""
    L = pkg.lib()
    assert L.mnt753_domain_vanishing_at(None, None, None) == -1
    assert L.mnt753_domain_lagrange_at(None, None, None, None) == -1 and b"lagrange_at" in L.mnt753_last_error()
    assert L.mnt753_vec_powers(2, None, None, 0, None) == -1
    assert L.mnt753_r1cs_qap_at(None, None, None, None, None, None, None, None, None) == -1 and b"qap_at" in L.mnt753_last_error()
    assert L.mnt753_r1cs_qap_plan(None, None) == -1


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]],
                         ids=["plain", "asan_ubsan"])
def test_transpose_builder_compiled_for_the_host(tmp_path, flags):
    """tools/host_qap_check.cpp over csrc/qap_transpose.hpp: the chunks partition every column's terms exactly once, none exceeds L,
    the work list goes by decreasing length -- on empty matrices, a single term, one full column, columns of L - 1, L, L + 1, 2 L + 1
    terms and duplicate (row, col) pairs"""
    exe = tmp_path / "host_qap_check"
    subprocess.run(["g++", "-std=c++17", *flags, "-o", str(exe), os.path.join(ROOT, "tools", "host_qap_check.cpp")], check=True, timeout=600)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ALL OK: 10 systems" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
