// TEST INFRASTRUCTURE -- not included by the product library.
// One dispatch over the device field primitives of fp753.hip.h / fp_inv.hip.h on raw limbs, exactly as a kernel holds them (no wire
// conversion, no normalisation on the way in or out), so that tests/ can drive every primitive at the edges of the contract stated
// above it.  Compiled twice from this one source: into the device hook mnt753_test_field_raw (mnt753_testhooks.hip) and, with g++,
// into a host twin (tools/host_tests/field_raw_host.cpp).  The exact reference and the edge generator are tests/field_raw_ref.py.
//
// A record: up to FR_OPS operands of NL limbs in, FR_OUT_WORDS words out = r0 (NL limbs) | r1 (NL limbs) | flag.
#pragma once
#include "fp_inv.hip.h"

namespace mnt753 {

constexpr int FR_OPS = 6;                      // operands per input record
constexpr int FR_IN_WORDS = FR_OPS * NL;
constexpr int FR_OUT_WORDS = 2 * NL + 1;
constexpr int FR_INV_GROUP_LANES = 16;         // FR_INV_GROUP: the group size of the pairing levels (MNT753_PAIR_INV_GROUP)

// op codes (mirrored by tests/field_raw_ref.py).  x0..x5 are the operands, k the scalar argument of the call.
enum FieldRawOp : int {
  FR_MUL = 0,          // r0 = fp_mul(x0, x1)
  FR_SQR,              // r0 = fp_sqr(x0)
  FR_MUL2,             // r0 = fp_mul2(x0, x1, x2, x3)
  FR_MUL3,             // r0 = fp_mul3(x0, x1, x2, x3, x4, x5)
  FR_REDUCE2P,         // r0 = fp_reduce2p(x0)
  FR_ADD,              // r0 = fp_add(x0, x1)
  FR_SUB,              // r0 = fp_sub(x0, x1)
  FR_NEG,              // r0 = fp_neg(x0)
  FR_HALF,             // r0 = fp_half(x0)
  FR_MUL_SMALL,        // r0 = fp_mul_small(x0, k)
  FR_MUL_S,            // r0 = fp_mul_s(x0, x1)
  FR_SQR_S,            // r0 = fp_sqr_s(x0)
  FR_MUL_S_IP,         // b = x1, a = x0; fp_mul_s_ip(b, a); r0 = b, r1 = a after the call
  FR_SQR_S_KEEP,       // a = x0; fp_sqr_s_keep(r0, a); r1 = a after the call
  FR_SUB_RAW,          // r0 = fp_sub_raw(x0, x1)
  FR_ADDSUB_RAW,       // r0 = fp_addsub_raw(x0, x1, subtract = k & 1)
  FR_NORM,             // r0 = fp_norm(x0)
  FR_RAW_MAYBE_ZERO,   // flag = fp_raw_maybe_zero(x0)
  FR_IS_ZERO,          // flag = fp_is_zero(x0)
  FR_CANON,            // r0 = fp_canon(x0)
  FR_INV,              // r0 = fp_inv(x0)
  FR_FROM_WIRE,        // r0 = fp_from_wire(words 0..23 of x0)
  FR_TO_WIRE,          // words 0..23 of r0 = fp_to_wire(x0)
  FR_NTT2,             // two carry-free butterfly stages of k_ntt_group (below)
  FR_INV_GROUP = 24,   // device only, whole waves: r0 = x0^-1 through the shared inversion of the pairing levels (fp_inv.hip.h), groups of
                       // FR_INV_GROUP_LANES consecutive records.  k = 0: fp_inv_lanes, every record its own inverse through ONE inversion
                       // per group (the residue of fp_inv(x0), canonical limbs not promised); k = 1: fp_inv_group itself, once per record
                       // of the group on that record's operand in every lane (the limbs of fp_inv(x0), bit for bit)
  FR_MUL_S_K,          // r0 = fp_mul_s_k(x0, x1): the limbs of FR_MUL_S           (mirrored by tests/mul_karatsuba_ref.py)
  FR_MUL_S_IP_K,       // b = x1, a = x0; fp_mul_s_ip_k(b, a); r0 = b, r1 = a after the call: the limbs of FR_MUL_S_IP
  FR_NUM_OPS
};

// Two stages of k_ntt_group's lazy butterflies (ntt_kernels.hip.h) on four elements x0..x3 with stage-A twiddle x4 and stage-B
// twiddle x5, in the kernel's order: stage A pairs (x0, x1) and (x2, x3) -- lo + t, lo - t with t = fp_mul_s(x4, hi), then
// fp_sub_raw and fp_addsub_raw; with k & 2, t = hi itself, as the first stage of a transform takes it (omega^0, no product) --
// and stage B pairs the two "+" outputs (k & 1 = 0) or the two "-" outputs (k & 1 = 1) of stage A, then fp_norm on both of its
// outputs.  k >> 2 picks what is returned in (r0, r1): 0 the stage-B inputs (stage-A outputs), 1 the stage-B outputs before
// normalisation, 2 the normalised outputs.
template <int M>
HD void field_raw_ntt2(Fp<M>& r0, Fp<M>& r1, const Fp<M> x[FR_OPS], uint32_t k) {
  Fp<M> t, lo[2], hi[2];
  for (int b = 0; b < 2; ++b) {
    const Fp<M>& xl = x[2 * b];
    const Fp<M>& xh = x[2 * b + 1];
    if (k & 2u) t = xh;
    else fp_mul_s(t, x[4], xh);
    fp_sub_raw(hi[b], xl, t);
    fp_addsub_raw(lo[b], xl, t, false);
  }
  Fp<M> yl = (k & 1u) ? hi[0] : lo[0], yh = (k & 1u) ? hi[1] : lo[1];
  if ((k >> 2) == 0) { r0 = yl; r1 = yh; return; }
  fp_mul_s(t, x[5], yh);
  fp_sub_raw(yh, yl, t);
  fp_addsub_raw(yl, yl, t, false);
  if ((k >> 2) == 1) { r0 = yl; r1 = yh; return; }
  fp_norm(r0, yl);
  fp_norm(r1, yh);
}

// One record: in = FR_IN_WORDS words, out = FR_OUT_WORDS words (every word written).
template <int M>
HD void field_raw_op(int op, const uint32_t* in, uint32_t k, uint32_t* out) {
  Fp<M> x[FR_OPS], r0, r1;
  uint32_t flag = 0;
  for (int j = 0; j < FR_OPS; ++j)
    for (int i = 0; i < NL; ++i) x[j].l[i] = in[j * NL + i];
  fp_zero(r0);
  fp_zero(r1);
  switch (op) {
    case FR_MUL: fp_mul(r0, x[0], x[1]); break;
    case FR_SQR: fp_sqr(r0, x[0]); break;
    case FR_MUL2: fp_mul2(r0, x[0], x[1], x[2], x[3]); break;
    case FR_MUL3: fp_mul3(r0, x[0], x[1], x[2], x[3], x[4], x[5]); break;
    case FR_REDUCE2P: fp_reduce2p<M>(r0, x[0].l); break;
    case FR_ADD: fp_add(r0, x[0], x[1]); break;
    case FR_SUB: fp_sub(r0, x[0], x[1]); break;
    case FR_NEG: fp_neg(r0, x[0]); break;
    case FR_HALF: fp_half(r0, x[0]); break;
    case FR_MUL_SMALL: fp_mul_small(r0, x[0], k); break;
    case FR_MUL_S: fp_mul_s(r0, x[0], x[1]); break;
    case FR_SQR_S: fp_sqr_s(r0, x[0]); break;
    case FR_MUL_S_IP: r0 = x[1]; fp_mul_s_ip(r0, x[0]); r1 = x[0]; break;
    case FR_SQR_S_KEEP: fp_sqr_s_keep(r0, x[0]); r1 = x[0]; break;
    case FR_SUB_RAW: fp_sub_raw(r0, x[0], x[1]); break;
    case FR_ADDSUB_RAW: fp_addsub_raw(r0, x[0], x[1], (k & 1u) != 0); break;
    case FR_NORM: fp_norm(r0, x[0]); break;
    case FR_RAW_MAYBE_ZERO: flag = fp_raw_maybe_zero(x[0]) ? 1u : 0u; break;
    case FR_IS_ZERO: flag = fp_is_zero(x[0]) ? 1u : 0u; break;
    case FR_CANON: fp_canon(r0, x[0]); break;
    case FR_INV: fp_inv(r0, x[0]); break;
    case FR_FROM_WIRE: fp_from_wire(r0, x[0].l); break;
    case FR_TO_WIRE: fp_to_wire(r0.l, x[0]); break;
    case FR_NTT2: field_raw_ntt2<M>(r0, r1, x, k); break;
    case FR_MUL_S_K: fp_mul_s_k(r0, x[0], x[1]); break;
    case FR_MUL_S_IP_K: r0 = x[1]; fp_mul_s_ip_k(r0, x[0]); r1 = x[0]; break;
    default: break;
  }
  for (int i = 0; i < NL; ++i) { out[i] = r0.l[i]; out[NL + i] = r1.l[i]; }
  out[2 * NL] = flag;
}

}  // namespace mnt753
