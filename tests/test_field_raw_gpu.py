"""GPU: the device field primitives on raw limbs (mnt753_test_field_raw over csrc/field_raw_ops.hip.h) against the exact reference of
tests/field_raw_ref.py -- the same records as tests/test_field_raw_cpu.py, every op at the edges of its stated contract -- and bit for
bit against the g++ build of the same dispatch, except where fp_norm is involved: hipcc contracts its float quotient estimate into an
FMA, so there the device may pick a different, equally valid representative and only residue and range are required.

Also the coordinate field of G2 on raw components (mnt753_test_ext_raw): Fq2 / Fq3 in the one-lane and the lane-split forms, every
component drawn from the edge set of [0, 2p), ragged batches (a partial last lane group; lane 63 of a wave idles in Fq3), against the
Fq2 / Fq3 arithmetic of tools/pyref.py, every output component in [0, 2p) with normalised limbs."""
import os
import random
import sys

import numpy as np
import pytest

import field_raw_ref as F

sys.path.insert(0, os.path.join(F.ROOT, "tools"))
import pyref  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host_twin(tmp_path_factory):
    return F.build_host_twin(tmp_path_factory.mktemp("field_raw_host"))


@pytest.mark.parametrize("mod", [0, 1])
@pytest.mark.parametrize("op", range(len(F.OP_NAMES)), ids=F.OP_NAMES)
def test_field_raw_device(gpu, host_twin, op, mod):
    dev = lambda m, o, rec, k: gpu.api.test_field_raw(m, o, rec, k)
    n = F.run_op(dev, mod, op, twin=host_twin)
    print(f"field_raw {F.OP_NAMES[op]} mod {mod}: {n} records checked on the device")


EXT_OPS = ("mul", "sqr", "inv", "is_zero")


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("curve", [0, 1])
def test_ext_raw_device(gpu, curve, split):
    C = pyref.Curve(curve)
    q, deg = C.q, C.deg
    mod = F.MODS.index(q)
    rinv = pow(F.RB, -1, q)
    rng = random.Random(77 + 2 * curve + split)
    # ragged: Fq2 split runs 2 lanes per element in 256-thread blocks, Fq3 split 21 elements per wave, 84 per block
    n = 389 if deg == 2 else 341
    comps = F.ext_case_components(mod, rng, 2 * n * deg)
    # elements that are zero with components 0 or p, and elements with one zero component
    for e in range(0, 24, 3):
        for c in range(deg):
            comps[e * deg + c] = rng.choice((0, q))
        comps[(e + 1) * deg + rng.randrange(deg)] = rng.choice((0, q))
    a_vals = [comps[e * deg:(e + 1) * deg] for e in range(n)]
    b_vals = [comps[(n + e) * deg:(n + e + 1) * deg] for e in range(n)]
    pack = lambda vals: np.array([sum((F.to_limbs(c) for c in el), []) for el in vals], dtype=np.uint32)
    A, B = pack(a_vals), pack(b_vals)
    mont = lambda el: tuple(c * rinv % q for c in el)          # the element a raw component tuple stands for
    T = gpu.api.test_ext_raw
    for op, name in enumerate(EXT_OPS):
        out = T(curve, split, op, A, B)
        assert out.shape == A.shape
        bad = []
        for e in range(n):
            x, y = mont(a_vals[e]), mont(b_vals[e])
            row = [int(w) for w in out[e]]
            if name == "is_zero":
                want = [int(C.f_is_zero(x))] + [0] * (deg * F.NL - 1)
                if row != want:
                    bad.append((e, "zero test"))
                continue
            if name == "inv" and C.f_is_zero(x):
                want = tuple(0 for _ in range(deg))
            else:
                want = C.f_mul(x, y) if name == "mul" else (C.f_mul(x, x) if name == "sqr" else C.f_inv(x))
            got = [row[c * F.NL:(c + 1) * F.NL] for c in range(deg)]
            for c in range(deg):
                v = F.val_std(got[c])
                if not F.normalised(got[c]) or not 0 <= v < 2 * q:
                    bad.append((e, f"component {c} outside [0, 2p)"))
                elif v * rinv % q != want[c]:
                    bad.append((e, f"component {c} wrong"))
        assert not bad, f"curve {curve} split {split} {name}: {len(bad)} of {n} wrong, first {bad[:5]}"
    print(f"ext_raw curve {curve} split {split}: {n} elements x {len(EXT_OPS)} ops checked")
