"""GPU: the signed product with a Karatsuba product half (csrc/fp753.hip.h: fp_mul_s_k, the forward sweep's running product in the
base-field k_pair_level, and its in-place form fp_mul_s_ip_k, the shared multiplier of the backward step loop) on raw limbs, through
the ops FR_MUL_S_K / FR_MUL_S_IP_K of mnt753_test_field_raw.

Per modulus one list of records, one launch per op: the edge vectors of the operand contract (tests/mul_karatsuba_ref.py: every limb
at 0, 2^28 - 1, +-(2^29 - 1); the halves at opposite extremes in both operands; the top limb at its negative end; 0, p, 2p - 1; both
argument orders) and 256 seeded random records.  The result must be, limb for limb,
  * what Python integers give for (a b + m p) / R', and
  * what FR_MUL_S (fp_mul_s, the product it replaces) returns for the same records on the same device;
the in-place form must also hand back the operand it keeps.  The level kernels that use the product are covered by the level tests
(test_inv_group_gpu.py, test_msm_occupancy_gpu.py, test_designed_points_gpu.py, test_msm_gpu.py, test_table_rows_gpu.py)."""
import random

import numpy as np
import pytest

import field_raw_ref as F
import mul_karatsuba_ref as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=[0, 1])
def raw(gpu, request):
    """(modulus, records, expected limbs from Python integers, FR_MUL_S's output) -- once per modulus, shared read-only"""
    mod = request.param
    p = F.MODS[mod]
    pairs = K.edge_pairs(p) + K.random_pairs(p, random.Random(8 + mod), 256)
    rec = K.records(pairs)
    want = K.expected_limbs(pairs, p)
    plain = gpu.api.test_field_raw(mod, F.MUL_S, rec, 0)
    for a in (rec, want, plain):
        a.setflags(write=False)
    assert len(pairs) % 64 != 0          # a ragged last wave
    return mod, rec, want, plain


@pytest.mark.parametrize("op", [K.OP_MUL_S_K, K.OP_MUL_S_IP_K], ids=["mul_s_k", "mul_s_ip_k"])
def test_karatsuba_product_limbs(gpu, raw, op):
    mod, rec, want, plain = raw
    got = gpu.api.test_field_raw(mod, op, rec, 0)
    n = rec.shape[0]
    bad = np.flatnonzero((got[:, :F.NL] != want).any(axis=1))
    assert bad.size == 0, f"modulus {mod}: {bad.size} of {n} records differ from the integer model, first at {bad[:8]}"
    bad = np.flatnonzero((got[:, :F.NL] != plain[:, :F.NL]).any(axis=1))
    assert bad.size == 0, f"modulus {mod}: {bad.size} of {n} records differ from fp_mul_s, first at {bad[:8]}"
    if op == K.OP_MUL_S_IP_K:
        assert np.array_equal(got[:, F.NL:2 * F.NL], rec[:, :F.NL]), f"modulus {mod}: the kept operand changed"
    else:
        assert not got[:, F.NL:].any()
