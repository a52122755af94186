"""The device field primitives on raw limbs, compiled for the host: the dispatch of csrc/field_raw_ops.hip.h built with g++
(tools/host_tests/field_raw_host.cpp) against the exact big-integer reference of tests/field_raw_ref.py, both moduli, every op at the
edges of the contract stated above its primitive (fp753.hip.h, fp_inv.hip.h) plus random records.  No GPU needed; the device build
of the same dispatch is held to the same contracts, and to this twin bit for bit, by tests/test_field_raw_gpu.py."""
import pytest

import field_raw_ref as F


@pytest.fixture(scope="module")
def host_twin(tmp_path_factory):
    return F.build_host_twin(tmp_path_factory.mktemp("field_raw_host"))


@pytest.mark.parametrize("mod", [0, 1])
@pytest.mark.parametrize("op", range(len(F.OP_NAMES)), ids=F.OP_NAMES)
def test_field_raw_host(host_twin, op, mod):
    n = F.run_op(host_twin, mod, op)
    print(f"field_raw {F.OP_NAMES[op]} mod {mod}: {n} records checked")
