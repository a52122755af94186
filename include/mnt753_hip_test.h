/* libmnt753_hip_test.so -- TEST INFRASTRUCTURE beside the product library (libmnt753_hip.so, include/mnt753_hip.h), which it links
 * against: the synthetic base points with known discrete logarithms that stand in for libsnark/generate_parameters.cpp on a box
 * with neither the reference nor its parameter files, and the device-level known-answer hooks under the MSM.  Loaded by tests/,
 * bench.py and __graft_entry__.smoke() only; main_hip and the B:: wrapper never see it (readelf -d: they need libmnt753_hip.so
 * alone). */
#ifndef MNT753_HIP_TEST_H
#define MNT753_HIP_TEST_H
#include "mnt753_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- deterministic synthetic inputs (host) ---------------------------------------------------------
 * Stand-in for libsnark/generate_parameters.cpp on machines that have neither the reference nor its
 * parameter files: bases with known discrete logarithms base[k] = e_k * G, uniform scalars, and the exact
 * value of sum scalars[k] * base[k] computed from the e_k (one scalar multiplication) for parity checks
 * at sizes no CPU implementation finishes quickly. */
int mnt753_synth_points(int curve, int group, uint64_t seed, size_t n, uint64_t* out_affine, int threads);
int mnt753_synth_expected_msm(int curve, int group, uint64_t seed, size_t n, const uint64_t* scalars, uint64_t* out_projective);
/* The group generator G as the library holds it (the GEN_* words of csrc/mnt753_generators.h, affine wire form, mnt753_affine_words
 * words; host only, no device needed).  It is also the stand-in point D of the batched-affine levels: a pair P, -P that cancels
 * leaves D in its slot and k_pair_fix subtracts fix_count * D from the bucket afterwards, so a base set that holds G or -G itself
 * meets D as an equal or an opposite point (tests/msm_occupancy.py, profile `collisions`). */
int mnt753_test_generator(int curve, int group, uint64_t* out_affine);

/* ---- test hooks (tests/ only; not used by the prover) -------------------------------------------------
 * The device field layer element-wise on n pairs of Fp elements in wire form (host pointers in and out), for known-answer
 * tests against libff's Fp_model (depends/libff/libff/algebra/fields/fp.tcc:161-186 mul_reduce, :405-417 +=, :491-508 -=,
 * :641-685 invert, :227-238 as_bigint).  mod: 0 = modulus A (Fr of MNT4753 / Fq of MNT6753), 1 = modulus B.
 * op: 0 a*b, 1 a+b, 2 a-b, 3 a^-1 (0 -> 0), 4 as_bigint(a), 5 -a, 6 a^2 (dedicated squaring), 7 wire->device->wire,
 * 8 a*b + a*a (fused two-product multiplier), 9 13*a (small-constant multiplier). */
int mnt753_test_field_op(int mod, int op, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out);
/* The coordinate field of G2 on the device, element-wise on n pairs of elements in wire form (c0 | c1 [| c2], host pointers):
 * Fq2 = Fq[u]/(u^2 - 13) on MNT4753 (depends/libff/libff/algebra/fields/fp2.tcc:79-90 mul, :118-126 squared, :129-142 inverse,
 * :58-70 + and -), Fq3 = Fq[u]/(u^3 - 11) on MNT6753 (fp3.tcc:83-96, :107-123, :126-143, :59-74).  split: 0 = the one-lane form
 * (Karatsuba through one multiplier instance), 1 = the lane-split form the G2 point kernels run (two / three lanes per element,
 * fused multi-product multipliers, ds_bpermute exchange).
 * op: 0 a*b, 1 a*a, 2 a^-1, 3 a+b, 4 a-b, 5 -a, 6 (a == b) as the element 1 or 0 (the zero test the kernels branch on). */
int mnt753_test_ext_op(int curve, int split, int op, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out);
/* The device field primitives on RAW limbs (csrc/field_raw_ops.hip.h), n records, host pointers: in holds 6 operands x 27 uint32
 * limbs per record exactly as a kernel holds them (no wire conversion: lazy ranges, un-normalised and signed limbs), out 2 x 27 limbs
 * plus one flag word per record.  k: the scalar argument of the op (fp_mul_small's multiplier, fp_addsub_raw's sign, the selector of
 * the NTT composite).  op: the FieldRawOp codes of field_raw_ops.hip.h.  The caller keeps every operand inside the contract stated
 * above the primitive in fp753.hip.h / fp_inv.hip.h. */
int mnt753_test_field_raw(int mod, int op, const uint32_t* in, size_t n, uint32_t k, uint32_t* out);
/* mnt753_test_ext_op on RAW components: 27 device limbs per component (c0 | c1 [| c2]) in and out, no wire conversion.
 * op: 0 a*b, 1 a*a, 2 a^-1, 3 is_zero(a) as 0 / 1 in limb 0 of component 0 (every other word 0). */
int mnt753_test_ext_raw(int curve, int split, int op, const uint32_t* a, const uint32_t* b, size_t n, uint32_t* out);
/* Every form of the group law the MSM kernels contain, on n pairs of points.  p_proj / q_proj / out_proj: projective X | Y | Z in
 * wire form (any representative; Z == 0 is the identity), host pointers.  group: MNT753_G1 / MNT753_G2; split (G2 only): 0 = one
 * lane per point, 1 = the lane-split configuration.  Reference: operator+ / mixed_add / dbl of mnt4753_G1 (depends/libff/libff/
 * algebra/curves/mnt753/mnt4753/mnt4753_g1.cpp:134-207, :265-313, :315-346), mnt4753_G2 (mnt4753_g2.cpp:150-223, :281-329,
 * :331-362), mnt6753_G1 (mnt6753_g1.cpp), mnt6753_G2 (mnt6753_g2.cpp:156-229, :287-335, :337-368).
 * op: 0 P + Q through the point VM (bucket reduction, edge merge);  1 2P through the VM (window table; equal points);
 *     2 P + Q with Q affine (Q's Z is taken as 1 unless 0) through the VM's mixed addition (bucket accumulation);
 *     3 the same as straight-line code (bucket accumulation of the base fields and the two-lane Fq2; other fields: as op 2);
 *     4 P + Q with two point-lanes per addition (narrow steps of the bucket reduction, edge merge of Fq3);
 *     5 P + Q as straight-line code (wide steps of the bucket reduction, base fields; other fields: as op 0);
 *     6 P + Q with one GROUP of lanes per addition (8 for the base fields, 16 for Fq2 / Fq3: the narrowest steps of the bucket
 *       reduction and the levels of the edge merge of a short lane list; split = 0 only). */
int mnt753_test_point_op(int curve, int group, int split, int op, const uint64_t* p_proj, const uint64_t* q_proj, size_t n, uint64_t* out_proj);

/* The target field of the pairing on the device (csrc/tower753.hip.h), element-wise on n pairs of elements in wire form (c0 | c1,
 * each an Fq2 / Fq3 element: mnt753_gt_words words; host pointers): Fq4 = Fq2[v]/(v^2 - u) on MNT4753 (depends/libff/libff/algebra/
 * fields/fp4.tcc), Fq6 = Fq3[v]/(v^2 - u) on MNT6753 (fp6_2over3.tcc).  split: 0 = over the one-lane coordinate field, 1 = over the
 * lane-split one, which the pairing kernels run.
 * op: 0 a*b, 1 a*a (complex squaring), 2 a^-1 (0 -> 0), 3 the unitary inverse, 4 a^|w0| (the power of the final exponent's last
 * chunk), 5 the whole final exponentiation of a, 10 + i the Frobenius map a^(q^i) for 1 <= i < k (k = 4 / 6). */
int mnt753_test_tower_op(int curve, int split, int op, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out);
/* The UNREDUCED Miller value of n pairs (affine wire-format points, neither the identity; host pointers): what
 * mnt{4,6}753_ate_miller_loop returns before final_exponentiation, mnt753_gt_words words per pair. */
int mnt753_test_miller_loop(int curve, int split, const uint64_t* g1_affine, const uint64_t* g2_affine, size_t n, uint64_t* out);
/* The two halves of the subgroup test of G2 (csrc/pairing_kernels.hip.h) on n points of the twist (affine
 * wire form, on the twist and not the identity, in G2 or not; host pointers), in the lane-split form the kernels run, so that a
 * failure of mnt753_check_subgroup can be placed in the endomorphism or in the stepping:
 * mnt753_test_g2_endomorphism: psi(P) = (x^q gamma_1^-2, y^q gamma_1^-3);
 * mnt753_test_g2_loop_multiple: [t - 1] P, t - 1 = q - r the signed ate loop count, by the doubling and addition steps of the Miller
 * loop alone; the identity (the incomplete steps ended with Z = 0) as zero words. */
int mnt753_test_g2_endomorphism(int curve, const uint64_t* g2_affine, size_t n, uint64_t* out_affine);
int mnt753_test_g2_loop_multiple(int curve, const uint64_t* g2_affine, size_t n, uint64_t* out_affine);
/* mnt753_groth16_verify_folded on host-memory proofs, inputs and coefficients with the parts of the fold handed out (host memory, any
 * may be NULL): out_f the UNREDUCED product of the Miller values of the stepped pairs (rho_i A_i, B_i)
 * (mnt753_gt_words words), out_s = rho ABC[0] + sum_j c_j ABC[j + 1] and out_t = sum rho_i C_i (affine wire form, 24 words each, the
 * identity as zero words), out_rho = sum rho_i as an element of Fr (wire form, 12 words).  status and accepted as there.  The parts are
 * filled whatever the verdict. */
int mnt753_test_fold_parts(const mnt753_vk* vk, const uint64_t* proofs, const uint64_t* inputs, size_t n, const uint64_t* coefficients, uint64_t* out_f,
                           uint64_t* out_s, uint64_t* out_t, uint64_t* out_rho, uint8_t* status, int* accepted);
/* mnt753_groth16_verify_folded_locate on host-memory proofs, inputs and coefficients with the parts of every SEGMENT handed out (host
 * memory, any of the out_ pointers and status may be NULL), one entry per segment, ceil(n /
 * mnt753_fold_segment_proofs(curve)) of them, in order: out_f the UNREDUCED product of the segment's stepped pairs' Miller values
 * (mnt753_gt_words words each), out_s = S_s and out_t = T_s (affine wire form, 24 words each, the identity as zero words), out_rho =
 * rho_s as an element of Fr (wire form, 12 words each), out_accepted the segment tail's answer (1 byte each: 1 accepted).  status: the
 * fold's status byte of every proof (n bytes: 0, 1, 3).  verdicts (n bytes, required), report and the return value as for the call
 * itself.  The parts are filled whatever the verdicts. */
int mnt753_test_fold_segment_parts(const mnt753_vk* vk, const uint64_t* proofs, const uint64_t* inputs, size_t n, const uint64_t* coefficients, uint64_t* out_f,
                                   uint64_t* out_s, uint64_t* out_t, uint64_t* out_rho, uint8_t* out_accepted, uint8_t* status, uint8_t* verdicts,
                                   mnt753_fold_locate_report* report);
/* chunks the calling thread's last mnt753_groth16_verify_folded_locate / mnt753_test_fold_segment_parts ran */
size_t mnt753_test_fold_locate_last_chunks(void);
/* milliseconds on the device (HIP events) of the stages of the calling thread's last mnt753_groth16_verify_folded / mnt753_test_fold_parts:
 * [0] the scaling and the point sum, [1] the Miller loops and the products, [2] the tail (0 where it was skipped).  tools/bench_fold.py. */
int mnt753_test_fold_last_timing(float out_ms[3]);
/* The input tables of a key (mnt753_vk_prepare_inputs).  _force_inputs_per_lane: every later call on the key
 * walks inputs_per_lane consecutive scalars per lane instead of the host's choice for the chunk (0: the host's choice again), so that a
 * test reaches the partial sums of several slices -- a ragged last slice, a single slice -- at a small number of proofs; values above
 * the number of scalars count as that number.  _last_timing: milliseconds on the device (HIP events) of [0] the walk and [1] the
 * segment sum with the normalisation of the key's last chunk, and [2] of the last build of the tables.  tools/bench_vk_inputs.py. */
int mnt753_test_vk_force_inputs_per_lane(mnt753_vk* vk, uint32_t inputs_per_lane);
int mnt753_test_vk_inputs_last_timing(const mnt753_vk* vk, float out_ms[3]);
/* Overwrites the key's e(alpha_g1, beta_g2) with gt_words (mnt753_gt_words words, host pointer; any words, canonical or not): the copy
 * on the device that every verification compares against and the host copy mnt753_vk_gt / _serialize read.  Nothing else of the key
 * changes.  For the near-miss tests of the accept / reject comparison (tests/test_pairing_designed_gpu.py): a key whose GT element
 * differs from the true one in one bit must reject the proof the true key accepts, whichever bit it is. */
int mnt753_test_vk_set_gt(mnt753_vk* vk, const uint64_t* gt_words);

/* The square root of csrc/fp_sqrt.hip.h on n raw field elements in wire form (host pointers): deg = 1 the base field Fq of the curve,
 * deg = 2 (MNT4753) / 3 (MNT6753) the coordinate field of G2, c0 | c1 [| c2].  The lane mapping is the product's (k_decompress): one
 * lane per base-field element, one lane group per extension element.  is_square[i] = 1 and out[i]^2 = in[i] (either root; 0 -> 0), or
 * is_square[i] = 0 and out[i] = 0.  _window: the same with the window of the fixed exponent chosen (1, 2 or 4; the product's is
 * SQRT_WINDOW) and, where ms is not NULL, the kernel's time on the device in milliseconds (HIP events; tools/bench_compress.py). */
int mnt753_test_field_sqrt(int curve, int deg, const uint64_t* in_wire, size_t n, uint64_t* out_wire, uint8_t* is_square);
int mnt753_test_field_sqrt_window(int curve, int deg, int window, const uint64_t* in_wire, size_t n, uint64_t* out_wire, uint8_t* is_square, float* ms);

/* mnt753_vec_dot (op 0: a = dev_a, b = dev_b) or mnt753_poly_eval (op 1: coefficients dev_a, t = host_t, dev_b unused) with at most
 * max_blocks blocks of 256 threads in the reducing launch (0: the device's own cap), so that a test reaches the second grid-stride trip
 * of a thread at a small n: one block covers 256 elements of a dot and 256 * 16 coefficients of a polynomial.  Device pointers, the
 * result on the host, as in the calls themselves. */
int mnt753_test_reduce_capped(int curve, int op, const uint64_t* dev_a, const uint64_t* dev_b, size_t n, const uint64_t* host_t, unsigned max_blocks,
                              uint64_t* host_out);

#ifdef __cplusplus
}
#endif
#endif /* MNT753_HIP_TEST_H */
