"""The folded verification equation in the Python-integer model of tests/fold_ref.py, on the committed g16
proofs of both curves.  No GPU.  tests/test_fold_gpu.py pins the device against the same model."""
import functools

import pytest

import fold_ref as FR

RHO = [0x9F3A7C2E51B84D06A1C3E5F708192A3B, 0x4D1E6F8092A3B4C5D6E7F8091A2B3C4D]   # fixed 128-bit coefficients


@functools.lru_cache(maxsize=None)
def batch(curve):
    """the fixture proof and a re-randomised copy of it, their inputs"""
    C = FR.model(curve).C
    _, _, _, _, proof, inp = FR.g16_words(curve)
    p0 = FR.proof_from_words(curve, proof)
    x = [C.fr_from_words([int(v) for v in inp])]
    return [p0, FR.rerandomised(curve, p0, 0x1234567)], [x, x]


@pytest.mark.parametrize("curve", [0, 1])
def test_the_fold_accepts_the_committed_proofs(curve):
    key = FR.g16_key(curve)
    proofs, inputs = batch(curve)
    assert all(FR.status(curve, p) == 0 for p in proofs)
    assert FR.accepts(key, proofs[:1], inputs[:1], RHO[:1])
    assert FR.accepts(key, proofs, inputs, RHO)
    # and the same with the smallest coefficient: rho = 1 is the per-proof equation itself
    assert FR.accepts(key, proofs[:1], inputs[:1], [1])


@pytest.mark.parametrize("curve", [0, 1])
def test_the_fold_rejects_a_replaced_c(curve):
    key = FR.g16_key(curve)
    proofs, inputs = batch(curve)
    A, B, _ = proofs[1]
    assert not FR.accepts(key, [proofs[0], (A, B, A)], inputs, RHO)
    assert not FR.accepts(key, [(proofs[0][0], proofs[0][1], proofs[0][0])], inputs[:1], RHO[:1])


@pytest.mark.parametrize("curve", [0, 1])
def test_cancelling_defects_pass_with_equal_coefficients_only(curve):
    """C_0 + D and C_1 - D: both proofs are wrong, their defects e(D, delta)^-1 and e(D, delta) cancel when rho_0 = rho_1.  This is why
    the coefficients must not be predictable, and it pins that they are applied at all."""
    C = FR.model(curve).C
    key = FR.g16_key(curve)
    proofs, inputs = batch(curve)
    D = C.mul(0xD15EA5E, C.gen(1), 1)
    bent = [(proofs[0][0], proofs[0][1], C.add(proofs[0][2], D, 1)), (proofs[1][0], proofs[1][1], C.add(proofs[1][2], C.neg(D), 1))]
    assert all(FR.status(curve, p) == 0 for p in bent)
    assert not FR.accepts(key, bent[:1], inputs[:1], [1]) and not FR.accepts(key, bent[1:], inputs[1:], [1])
    assert FR.accepts(key, bent, inputs, [1, 1])
    assert not FR.accepts(key, bent, inputs, [1, 2])
