/* mnt753_hip.h -- C ABI of libmnt753_hip.so: the MI355X (gfx950) implementation of the Groth16 prover
 * hot path of MinaProtocol/snark-challenge-prover-reference (MSM over G1/G2 and radix-2 FFT over Fr of
 * MNT4753 / MNT6753).
 *
 * This is the drop-in boundary.  Each entry point names the reference interface it replaces
 * (paths relative to the reference tree).  The C++ class pair mnt4753_hip / mnt6753_hip in
 * include/prover_hip_functions.hpp mirrors libsnark/prover_reference_include/prover_reference_functions.hpp
 * member for member on top of this ABI; INTEGRATION.md shows the reference-side binding.
 *
 * Data formats (identical to the reference's files, libsnark/serialization.hpp:22-121):
 *   Fr / Fq element : 12 little-endian uint64 limbs, Montgomery form with R = 2^768, fully reduced.
 *   G1 affine       : x | y                      (24 u64);  y == 0 encodes the identity.
 *   G2 affine       : x.c0 | x.c1 [| x.c2] | y.c0 | y.c1 [| y.c2]   (48 u64 MNT4753, 72 u64 MNT6753).
 *   projective      : X | Y | Z  (homogeneous projective, identity = (0 : 1 : 0)) -- the in-memory form
 *                     of libff::mnt4753_G1 (depends/libff/libff/algebra/curves/mnt753/mnt4753/mnt4753_g1.hpp).
 *
 * Conventions: every function returns 0 on success and a negative MNT753_E* code on failure;
 * mnt753_last_error() returns a message for the calling thread's last failure.  Pointers named dev_*
 * are HIP device pointers (e.g. torch tensor.data_ptr(), or mnt753_dev_alloc); all others are host
 * pointers.  `stream` is a hipStream_t passed as void* (NULL = default stream).  One context per
 * process; calls are serialised by the caller (same threading contract as the reference wrapper).
 * There is NO CPU fallback: without a HIP device every compute entry point returns MNT753_ENODEV.
 */
#ifndef MNT753_HIP_H
#define MNT753_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MNT753_CURVE_MNT4753 0
#define MNT753_CURVE_MNT6753 1
#define MNT753_G1 1
#define MNT753_G2 2

#define MNT753_OK 0
#define MNT753_EINVAL (-1)   /* bad argument (null pointer, size, curve / group id) */
#define MNT753_ENODEV (-2)   /* no HIP device / library not initialised */
#define MNT753_EHIP (-3)     /* a HIP runtime call failed */
#define MNT753_ENOMEM (-4)   /* device or host allocation failed */
#define MNT753_EDOMAIN (-5)  /* no supported evaluation domain of this size for this field */
#define MNT753_ESELFTEST (-6) /* mnt753_self_test: a known-answer check failed -- this build must not be used to prove */

/* FFT kinds: libfqfft basic_radix2_domain::{FFT,iFFT,cosetFFT,icosetFFT}
 * (depends/libfqfft/libfqfft/evaluation_domain/domains/basic_radix2_domain.tcc:62-96);
 * the coset shift is Fr::multiplicative_generator as in libsnark/prover_reference_functions.cpp:227-238. */
#define MNT753_FFT 0
#define MNT753_IFFT 1
#define MNT753_COSET_FFT 2
#define MNT753_ICOSET_FFT 3

/* ---- lifecycle ------------------------------------------------------------------------------ */
/* replaces B::init_public_params (prover_reference_functions.hpp:25).  device = HIP device ordinal. */
int mnt753_init(int device);
/* Several GPUs in one process: logical devices 0 .. n-1 = HIP devices 0 .. n-1.  A base set, a domain
 * or a buffer lives on the device that is current for the calling thread when it is created (mnt753_set_device; device 0
 * after initialisation, also in new threads); entry points that take a base set run on that set's device whatever the
 * current one is.  The reference shards an MSM over OpenMP threads as contiguous slices and sums the partial results
 * serially (depends/libff/libff/algebra/scalar_multiplication/multiexp.tcc:417-440); the wrapper classes do the same over
 * devices: one base set per device and slice; every device streams its own slice of the witness from the input file
 * (mnt753_load_file_to_device on that device), only the slices of coefficients_for_H travel device 0 -> device g
 * (mnt753_copy_peer_async, xGMI); one projective point back per device, folded on the host in rank order with mnt753_point_add.
 * MNT753_SHARE_DEVICE=1 (development) maps the logical devices onto however many are visible. */
int mnt753_init_devices(int n_devices);
/* Known-answer self-test of THIS build on the current device: expected words computed by the reference's own code (libff's
 * multi_exp_with_mixed_addition, libfqfft's compute_H call sequence, libff's group classes) are embedded in the library as constants
 * (csrc/mnt753_selftest_data.h, minted by tools/gen_selftest_data.py through oracle/_ref -- data, none of the oracle's code).
 * level 0: the host tails (point decoding, addition, doubling, affine output) on one libff record per group; level 1: plus a 256-point
 * MSM per (curve, group) -- with and without the batched-affine levels of the large sets in front of it -- and compute_H on a 2^8
 * domain per curve (~0.15 s for both curves, most of it the allocations of the small base sets); level 2: plus the same MSMs over a window table (~0.35 s).  0 if everything agrees, MNT753_ESELFTEST (and
 * a message naming the check) if one word differs, another code if a call failed.  Why: a proof is only as sound as the build that
 * computed it, and the compiler has miscompiled kernels of this library before; the reference carries a check of the same
 * purpose around its prover (libsnark/main.cpp:295-343).  B::init_public_params runs level 1 for its curve once per process (MNT753_SELFTEST=0
 * skips it, MNT753_SELFTEST=2 raises it); `main_hip <curve> self-test` runs level 2. */
int mnt753_self_test(int level);
/* the same for one curve (MNT753_CURVE_MNT4753 / MNT753_CURVE_MNT6753): what B::init_public_params of that curve's class runs */
int mnt753_self_test_curve(int curve, int level);
int mnt753_device_count(void);
int mnt753_set_device(int logical_device);
int mnt753_get_device(void);   /* the calling thread's current logical device (0 before mnt753_set_device) */
/* Peer access: after the call the copy engines and kernels of `device` may address the memory of `peer` directly
 * (hipDeviceEnablePeerAccess), so that a copy between the two goes over their xGMI link instead of staging through host memory.
 * *how (may be NULL) = MNT753_PEER_SAME (both logical devices are one GPU: MNT753_SHARE_DEVICE), MNT753_PEER_DIRECT, or
 * MNT753_PEER_STAGED (the platform offers no peer access for the pair; copies still work, through the host).  Idempotent.
 * mnt753_init_devices asks for every ordered pair; the wrapper asks again and says under MNT753_TRACE=1 what it got.  The one-GPU
 * reference has nothing to compare (cuda_prover_piecewise.cu:24-34 keeps ca / cb / cc on one device); this is what the sharding of
 * SURVEY.md section 8e adds.  A mnt753_copy_peer_async is a command of the DESTINATION's default queue: the destination's copy
 * engine (ROCr's SDMA; a blit kernel on its CUs where SDMA is turned off) reads the source's memory over the link. */
enum { MNT753_PEER_SAME = 0, MNT753_PEER_DIRECT = 1, MNT753_PEER_STAGED = 2 };
int mnt753_enable_peer_access(int device, int peer, int* how);
int mnt753_copy_peer(int dst_device, void* dev_dst, int src_device, const void* dev_src, size_t bytes);
/* The same without blocking the host: the copy is enqueued on dst_device's default stream and starts after everything enqueued so
 * far on src_device's default stream (an event recorded there, waited for on the destination) -- how the slices of
 * coefficients_for_H leave device 0 behind compute_H (cuda_prover_piecewise.cu:79-81) while the host goes on enqueueing.  An MSM
 * started afterwards on dst_device with stream == NULL (mnt753_msm_start) is ordered behind the copy. */
int mnt753_copy_peer_async(int dst_device, void* dev_dst, int src_device, const void* dev_src, size_t bytes);
/* The exchange of a sharded MSM over RCCL ("Collective"): every logical device contributes `words` u64 -- its
 * partial points, multiexp.tcc:417-431 lifted to devices --, host_in[g] being device g's block in host memory (where mnt753_msm_finish
 * put it); afterwards host_out holds the n_devices blocks in rank order, ready for the serial fold of multiexp.tcc:433-438
 * (mnt753_point_add).  A single-process communicator over the devices of mnt753_init_devices (ncclCommInitAll), one ncclAllGather per
 * device in a group call, xGMI between the GPUs; librccl is loaded on first use.  MNT753_ENODEV if librccl cannot be loaded or the
 * logical devices are not distinct GPUs (MNT753_SHARE_DEVICE).  The wrapper classes fold on the host by default -- a partial point
 * arrives there anyway -- and take this path with MNT753_FOLD=rccl (main_hip --fold rccl). */
int mnt753_exchange_points(const uint64_t* const* host_in, size_t words, uint64_t* host_out);
double mnt753_exchange_last_us(void);   /* duration of the last exchange: staging, collective, copy back */
const char* mnt753_last_error(void);
/* number of words (uint64) of one element / point of the given kind */
size_t mnt753_affine_words(int curve, int group);      /* 24, 48 (MNT4753 G2) or 72 (MNT6753 G2) */
size_t mnt753_projective_words(int curve, int group);  /* 36, 72 or 108 */

/* ---- device memory helpers (for hosts that do not bring their own allocator) ------------------- */
int mnt753_dev_alloc(void** dev_ptr, size_t bytes);
int mnt753_dev_free(void* dev_ptr);
int mnt753_copy_h2d(void* dev_dst, const void* src, size_t bytes);
int mnt753_copy_d2h(void* dst, const void* dev_src, size_t bytes);
int mnt753_copy_d2d(void* dev_dst, const void* dev_src, size_t bytes);
int mnt753_dev_memset(void* dev_dst, int value, size_t bytes);
int mnt753_sync(void* stream);
/* free / total memory of the calling thread's current device (hipMemGetInfo): the wrapper prints what a parameter set occupies
 * (window tables, workspaces, the pooled buffers of the batched-affine levels) under MNT753_TRACE_LOAD=1 */
int mnt753_dev_mem_info(size_t* free_bytes, size_t* total_bytes);
/* Stream `bytes` of file `path` starting at `file_offset` into device memory (double-buffered pinned staging, reads
 * overlap the H2D copies); blocks the calling thread until the data is on the device.  Thread-safe: the wrapper's input
 * loader calls it from a background thread while the main thread launches kernels (replaces the 6.3 M fread calls of
 * the reference's groth16_input constructor, prover_reference_functions.cpp:48-76). */
int mnt753_load_file_to_device(const char* path, size_t file_offset, size_t bytes, void* dev_dst);

/* ---- MSM --------------------------------------------------------------------------------------
 * A base set is the device-resident, pre-converted image of a vector_G1 / vector_G2 of the parameters
 * (B::params_A/B1/L/H/B2, prover_reference_functions.hpp:66-70).  The reference loads parameters before
 * its timing window opens (libsnark/main.cpp:201-203); creating a base set belongs to that phase. */
typedef struct mnt753_bases mnt753_bases;
/* affine: n points in the wire format above; on_device != 0 if `affine` is a device pointer */
int mnt753_bases_create(int curve, int group, const uint64_t* affine, int on_device, size_t n, mnt753_bases** out);
int mnt753_bases_free(mnt753_bases* b);
size_t mnt753_bases_size(const mnt753_bases* b);

/* replaces B::multiexp_G1 / B::multiexp_G2 (prover_reference_functions.hpp:49-52):
 *   result = sum_{i < n} scalars[i] * bases[base_offset + i]
 * scalars: n Fr elements, wire format (Montgomery), device pointer if scalars_on_device != 0.
 * out_projective: host buffer of mnt753_projective_words() u64 -- X | Y | Z, Montgomery, fully reduced
 * (NOT normalised to Z = 1; feed it to mnt753_point_to_affine / mnt753_point_add). */
int mnt753_msm(mnt753_bases* b, size_t base_offset, const uint64_t* scalars, int scalars_on_device, size_t n,
               uint64_t* out_projective, void* stream);
/* The same, asynchronous: _start enqueues every kernel of the MSM and returns; _finish waits for it and writes the
 * result.  stream == NULL uses a non-blocking stream owned by the base set, ordered after all work already enqueued on
 * the default stream -- so the five MSMs of one proof (A, B1, B2, L, H: independent, cuda_prover_piecewise.cu:71-81) run
 * concurrently and the latency-bound reduction tail of one overlaps the bucket accumulation of another.  At most one
 * MSM may be in flight per base set. */
int mnt753_msm_start(mnt753_bases* b, size_t base_offset, const uint64_t* scalars, int scalars_on_device, size_t n, void* stream);
int mnt753_msm_finish(mnt753_bases* b, uint64_t* out_projective);
/* Order the throughput phases of two MSMs that are in flight together: the point kernels (pairing levels, accumulate: the ones that
 * fill the chip) of b's NEXT mnt753_msm_start begin when those of `first`'s latest mnt753_msm_start have ended; b's sort still runs
 * as early as it can.  Without it the two interleave, finish together, and both latency-bound tails (edge merge, bucket reduction:
 * 1.3 - 3 ms of a 2^20-point MSM during which the chip idles) end the prove; with it first's tail runs under b's point kernels and
 * only b's is left -- so the MSM with the shortest tail goes last (A behind C in the prove: cuda_prover_piecewise.cu:71-81 starts
 * them in an order that does not matter there).  Worth 1 - 3 % for the small sets (MNT6753 2^15: 15.7 -> 15.2 and 15.3 -> 15.2 ms per proof in two series); two
 * 2^20-point MSMs gain more from filling each other's kernel ends interleaved (measured 157.2 -> 158.4 ms ordered), so the wrapper
 * orders only below 2^18 points.  Both sets on one device; call it after first's mnt753_msm_start.  The order refers to first's
 * latest start AT THE TIME b starts; it is dropped (no wait) if `first` is freed before b's next start. */
int mnt753_msm_order_after(mnt753_bases* b, const mnt753_bases* first);

/* Window tables of the base sets created FROM NOW ON: mode 1 (default) -- a set of 4096 points or more gets the table of its window
 * multiples 2^(cw) P_i at creation (0.33 s of kernels per 2^20 G1 points, 1.3 s for 2^20 G2 points; an MSM over it then takes
 * 23.7 ms instead of 38-43); mode 0 -- no tables and no batched-affine levels (whose buffers are tens of GB to allocate): what a
 * process that will prove ONCE wants, because the reference's CLI is such a
 * process (libsnark/main.cpp:196-203 loads the parameters per invocation, :274-293) and a table never pays for itself in one proof.
 * The wrapper's B::one_shot / main_hip's default for a single job use it.  MNT753_MSM_PRECOMP=0 / 1 in the environment overrides
 * both.  Returns the previous mode. */
int mnt753_msm_set_window_table(int mode);
/* window size override (0 = automatic); returns previous value.  Tuning knob, not part of the reference. */
int mnt753_msm_set_window_bits(int c);
/* time of the last mnt753_msm call's kernels in milliseconds (HIP events on the launch stream):
 * index 0 = total, 1 = digits+sort, 2 = bucket accumulation kernel, 3 = bucket reduction, 4 = host tail */
int mnt753_msm_last_timing(float out_ms[5]);
/* plan of the last mnt753_msm call: [0] window bits c, [1] windows W, [2] 1 if the precomputed window table was used,
 * [3] sorted entries per accumulate lane T */
int mnt753_msm_last_plan(int out[4]);
/* Levels of the batched-affine pairing pass the last G1 MSM ran before its accumulate kernel (0 = none). */
int mnt753_msm_last_pair_levels(void);
/* irregular pairing levels the last MSM ran behind the regular ones (csrc/msm_kernels.hip.h, "irregular levels") */
int mnt753_msm_last_irr_levels(void);

/* ---- small group operations on the host (O(1) work per proof) ------------------------------------ */
/* replaces B::G1_add (hpp:32) */
int mnt753_point_add(int curve, int group, const uint64_t* a_proj, const uint64_t* b_proj, uint64_t* out_proj);
/* replaces B::G1_scale (hpp:33): scalar is an Fr element in wire (Montgomery) form */
int mnt753_point_scale(int curve, int group, const uint64_t* scalar, const uint64_t* p_proj, uint64_t* out_proj);
/* to_affine_coordinates + write_g1/write_g2 encoding (serialization.hpp:44-67): identity -> all zero */
int mnt753_point_to_affine(int curve, int group, const uint64_t* p_proj, uint64_t* out_affine);
/* read_g1 / read_g2 decoding (serialization.hpp:84-111): y == 0 -> identity */
int mnt753_point_from_affine(int curve, int group, const uint64_t* affine, uint64_t* out_proj);

/* ---- fixed-base batch scalar multiplication ---------------------------------------------------------------
 * n scalars times ONE base point: libff's get_window_table / windowed_exp / batch_exp / batch_exp_with_coeff followed by
 * batch_to_special (depends/libff/libff/algebra/scalar_multiplication/multiexp.tcc:547-583, :585-612, :614-668, :670-720) -- what the
 * Groth16 generator applies to its A, B, L, H and IC queries (libsnark/zk_proof_systems/ppzksnark/r1cs_gg_ppzksnark/
 * r1cs_gg_ppzksnark.tcc:293-352).  The table holds, for every window j of w bits, the multiples m 2^(jw) P, m = 1 .. 2^(w-1) (signed
 * digits: half of libff's 2^w rows per window); one lane walks one scalar through it (csrc/batch_exp_kernels.hip.h, DESIGN.md
 * section 4.9). */
typedef struct mnt753_fixed_base mnt753_fixed_base;
/* get_window_table (multiexp.tcc:547-583) for ONE base point, on the calling thread's current device, with the workspace of one
 * pass.  point: host pointer, affine wire format (y == 0: the identity -- no table is built, every output is the identity).
 * window_bits: 0 = chosen by the library (the widest table within the 256 MiB Infinity Cache), else 2 .. 22.
 * tile: scalars per pass, 0 = automatic (2^17); rounded up to a multiple of the inversion batch, at most 2^24.
 * The width and the tile belong to the object: there is no process-wide setting and no environment variable.
 * MNT753_EINVAL: bad ids, a null pointer, a width out of range.  MNT753_ENOMEM: the table (or the workspace) does not fit. */
int mnt753_fixed_base_create(int curve, int group, const uint64_t* point, int window_bits, size_t tile, mnt753_fixed_base** out);
int mnt753_fixed_base_free(mnt753_fixed_base* fb);
/* [0] window bits w, [1] windows W = ceil(754 / w), [2] results per field inversion B, [3] scalars per pass T */
int mnt753_fixed_base_plan(const mnt753_fixed_base* fb, int out[4]);
size_t mnt753_fixed_base_table_bytes(const mnt753_fixed_base* fb);
/* batch_exp / batch_exp_with_coeff followed by batch_to_special (multiexp.tcc:614-720):
 *   out_affine[i] = (coeff * scalars[i]) * P,  i < n,  affine wire format, identity = all words zero
 * -- word for word what mnt753_point_to_affine(mnt753_point_scale(..)) gives, so a device output can go straight into
 * mnt753_bases_create(.., on_device = 1, ..).  scalars: n canonical Fr elements in wire form, only read (the product with the
 * coefficient goes into the object's workspace).  host_coeff: one Fr element in HOST memory, or NULL for 1.  out_affine must not
 * overlap scalars.  n = 0 succeeds and writes nothing.  The workspace is sized by T, not by n: longer inputs run in passes, and no
 * call allocates.  Streams as for mnt753_fft: with both ends on the device the call only enqueues on `stream`; with an end in host
 * memory it returns when that end is done.  One call in flight per object. */
int mnt753_batch_exp(mnt753_fixed_base* fb, const uint64_t* scalars, int scalars_on_device, size_t n, const uint64_t* host_coeff,
                     uint64_t* out_affine, int out_on_device, void* stream);
/* milliseconds from HIP events: [0] the table build of mnt753_fixed_base_create, [1] the walk and [2] the normalisation of the LAST
 * pass of the last mnt753_batch_exp call (the whole call when n <= T); waits for that pass.  Zeros before the first call. */
int mnt753_fixed_base_last_timing(mnt753_fixed_base* fb, float out_ms[3]);

/* ---- FFT over Fr ---------------------------------------------------------------------------------- */
typedef struct mnt753_domain mnt753_domain;
/* libfqfft's basic_radix2_domain of exactly m elements: the constructor accepts every power of two m <= 2^s (s = 30 MNT4753,
 * 15 MNT6753), MNT753_EDOMAIN otherwise.  2^25 (MNT4753) is the largest size compared with the reference -- every schedule of
 * the transform kernel up to its first four-launch one, tests/test_fft_schedules_gpu.py; nothing above it has been run.  A domain
 * holds 544 bytes of device memory per element (two twiddle tables of m / 2 and three coset tables of m entries of 112 bytes, a
 * work vector of m elements of 96): 18.3 GB at 2^25, beside the caller's vectors of 96 bytes per element.
 * (B::get_evaluation_domain goes through mnt753_domain_create_for.) */
int mnt753_domain_create(int curve, size_t m, mnt753_domain** out);
/* replaces B::get_evaluation_domain (hpp:30) = libfqfft get_evaluation_domain(min_size): the first of basic_radix2_domain,
 * extended_radix2_domain (2^(s+1): two size-2^s transforms, the second on the coset shift * <omega>) and step_radix2_domain
 * (2^k + 2^r) that accepts min_size, then the same three at big + rounded_small, which may be larger than min_size
 * (mnt753_domain_size says).  Every call that takes a domain works on all kinds.  MNT753_EDOMAIN, with a message naming
 * the size and the reference's domain, wherever the reference's walk stops at a domain this library does not build: a
 * mixed-radix basic domain (MNT6753 only: its Fr accepts 2^a 5^b, a <= 15, b <= 2, so 5, 10, 25, 40, 5 * 2^15 are refused,
 * not stepped) or the candidates behind the first six (mixed-radix best fit, geometric and arithmetic sequence domains). */
#define MNT753_DOMAIN_BASIC 0
#define MNT753_DOMAIN_EXTENDED 1
#define MNT753_DOMAIN_STEP 2
#define MNT753_DOMAIN_MIXED 3
int mnt753_domain_create_for(int curve, size_t min_size, mnt753_domain** out);   /* == mnt753_domain_create_for_ex(curve, min_size, 0, out) */
/* The same walk with the mixed-radix basic domains of MNT6753 built instead of refused (flags = MNT753_DOMAIN_ALLOW_MIXED): wherever
 * the walk above stops at "a mixed-radix basic_radix2_domain" -- candidates 1 and 4 (the basic domain at min_size or at big +
 * rounded_small) and candidate 7 (best_mixed_domain_size, get_evaluation_domain.tcc:35-56, 110-118: the smallest 2^a 5^b >= min_size,
 * which may be larger than min_size) -- it returns a domain of kind MNT753_DOMAIN_MIXED.  That reaches 25 * 2^15 = 819200 on MNT6753,
 * where the radix-2 kinds end at 2^16.  Still refused, with the same messages: an extended domain over a mixed-radix half, the
 * sequence domains, sizes 0 and 1.  The flag is an argument of the call, there is no process-wide switch; it changes nothing on
 * MNT4753, whose Fr has no small subgroup.  Unknown flag bits: MNT753_EINVAL. */
#define MNT753_DOMAIN_ALLOW_MIXED 1u
int mnt753_domain_create_for_ex(int curve, size_t min_size, unsigned flags, mnt753_domain** out);
/* libfqfft's basic_radix2_domain of exactly m = 2^a 5^b elements, 0 <= a <= 15, 1 <= b <= 2, on MNT6753 (mnt6753_init.cpp:73-76
 * declares the small subgroup of order 5^2; basic_radix2_domain.tcc:26-60 accepts, basic_radix2_domain_aux.tcc:46-165 transforms):
 * the exact-size sibling of mnt753_domain_create, which keeps the powers of two.  MNT753_EDOMAIN for any other size and for every
 * size on MNT4753.  omega = get_root_of_unity(m) (field_utils.tcc:59-70), the coset shift g = 17 as in the other kinds.  The
 * transform is the m / 5^b-point radix-2 transform of a basic domain, 5^b times, and b radix-5 passes (csrc/ntt_kernels.hip.h,
 * DESIGN.md section 4.5).  Device memory: 544 bytes per element (the powers of omega, omega^-1, g and g^-1, m entries of 112
 * bytes each, and a work vector of m elements of 96) plus the inner radix-2 domain of m / 5^b elements at 208 bytes each: 586 bytes
 * per element for b = 1, 552 for b = 2 -- 480 MB at 819200. */
int mnt753_domain_create_mixed(int curve, size_t m, mnt753_domain** out);
int mnt753_domain_kind(const mnt753_domain* d);      /* MNT753_DOMAIN_*; -1 for a null domain */
int mnt753_domain_free(mnt753_domain* d);
size_t mnt753_domain_size(const mnt753_domain* d);   /* B::domain_get_m (hpp:47) */
/* replaces B::domain_iFFT / domain_cosetFFT / domain_icosetFFT (hpp:42-45) and libfqfft FFT; in place on
 * a device vector of m Fr elements in wire format.  The transforms of one domain share its work buffer: calls on different
 * streams are ordered on the device one after the other (an event per domain); host threads must not enter the same domain
 * at the same time. */
int mnt753_fft(mnt753_domain* d, int kind, uint64_t* dev_vec, void* stream);
/* replaces B::domain_divide_by_Z_on_coset (hpp:46) */
int mnt753_divide_by_z_on_coset(mnt753_domain* d, uint64_t* dev_vec, void* stream);
/* replaces B::vector_Fr_muleq / vector_Fr_subeq (hpp:35-36): a[i] = a[i] (*|-) b[i], i < n.  dev_b may be dev_a itself, as in
 * the reference's loops (the squares in place / all zeros); otherwise the two vectors must not overlap. */
int mnt753_vec_muleq(int curve, uint64_t* dev_a, const uint64_t* dev_b, size_t n, void* stream);
int mnt753_vec_subeq(int curve, uint64_t* dev_a, const uint64_t* dev_b, size_t n, void* stream);
/* dst[i] = src[i] * k, i < n, k one Fr element in HOST memory (wire format); dst may be src.  Used to fold the factor r of
 * r * Bt1 (cuda_prover_piecewise.cu:85-87: B::G1_scale(B::input_r(inputs), evaluation_Bt1)) into the scalars of that sum, so that
 * Ht + Lt + r Bt1 becomes one multi-scalar multiplication (B::groth16_C, include/prover_hip_functions.hpp). */
int mnt753_vec_scale(int curve, uint64_t* dev_dst, const uint64_t* dev_src, const uint64_t* host_scalar, size_t n, void* stream);
/* the whole of compute_H (cuda_prover_piecewise.cu:18-53) resident on the device:
 * dev_ca / dev_cb / dev_cc hold m elements each and are overwritten; dev_h receives m + 1 elements
 * (coefficients_for_H, last entry 0). */
int mnt753_compute_h(mnt753_domain* d, uint64_t* dev_ca, uint64_t* dev_cb, uint64_t* dev_cc, uint64_t* dev_h,
                     void* stream);
/* The two halves of compute_H, for a prover that spreads it over the devices of a node (task parallelism, SURVEY.md section 8e: the
 * transform is not sharded, but ca, cb and cc are independent until the pointwise step, cuda_prover_piecewise.cu:24-34):
 *   _chain : x <- cosetFFT(iFFT(x)) in place on one vector of m elements (:24-27 for ca / cb, :33-34 for cc);
 *   _finish: a <- icosetFFT((a * b - c) / Z), h <- a | 0 (:29-47); b and c are only read.
 * A domain (its tables and work buffer) lives on the device that was current when it was created; both calls run there whatever the
 * calling thread's current device is, and every vector handed to them must be on that device (mnt753_copy_peer_async brings the
 * chained cb / cc from the devices that transformed them).  mnt753_compute_h == three _chain + one _finish on one device. */
int mnt753_compute_h_chain(mnt753_domain* d, uint64_t* dev_vec, void* stream);
int mnt753_compute_h_finish(mnt753_domain* d, uint64_t* dev_a, const uint64_t* dev_b, const uint64_t* dev_c, uint64_t* dev_h, void* stream);
int mnt753_domain_device(const mnt753_domain* d);   /* logical device the domain lives on */
/* ---- the domain at a point: what a Groth16 generator needs of it ------------------------------------
 * t: one canonical Fr element in HOST memory, wire form; t >= r is MNT753_EINVAL and nothing is enqueued.  All kinds of domain.
 * replaces evaluation_domain::compute_vanishing_polynomial(t) (t^m - 1 for basic and mixed domains; extended_radix2_domain.tcc:155-158,
 * step_radix2_domain.tcc:230-233): host arithmetic, a handful of products; host_zt receives one element. */
int mnt753_domain_vanishing_at(mnt753_domain* d, const uint64_t* host_t, uint64_t* host_zt);
/* replaces evaluation_domain::evaluate_all_lagrange_polynomials(t) (basic_radix2_domain_aux.tcc:333-395 for basic and mixed domains,
 * extended_radix2_domain.tcc:120-139, step_radix2_domain.tcc:189-214): dev_u receives the m = mnt753_domain_size(d) values L_i(t), the
 * same words the reference computes, also where t is an element of the domain (the indicator vector of its index, as the reference
 * returns it) and for t = 0.  The m inversions of the reference are one inversion per 16 elements on the device (csrc/qap_kernels.hip.h);
 * the few scalars of a call are computed on the host.  The first call allocates a workspace of 112 bytes per element that stays with
 * the domain; later calls only enqueue on `stream`.  The workspace is shared like the work buffer of mnt753_fft: calls on one domain
 * (this one and the transforms) on different streams are ordered on the device, and host threads must not enter the same domain at
 * the same time -- calls on one domain are not concurrent. */
int mnt753_domain_lagrange_at(mnt753_domain* d, const uint64_t* host_t, uint64_t* dev_u /* d->m elements */, void* stream);
/* dev_out[i] = t^i, i < n: the Ht of r1cs_to_qap.tcc:155-159.  n = 0 succeeds and writes nothing. */
int mnt753_vec_powers(int curve, const uint64_t* host_t, uint64_t* dev_out, size_t n, void* stream);   /* 1, t, ..., t^(n-1) */

/* ---- reductions over Fr and the spot check of compute_H: H(t) Z(t) = A(t) B(t) - C(t) at one point -------
 * The reducing calls return their result to HOST memory in canonical wire form and wait for `stream`; the vectors are device memory
 * on the calling thread's current device (domain calls: on the domain's device).  Results do not depend on the launch geometry.
 * A device keeps 340 KB of partial sums from its first reduction on; reductions on one device take turns.
 * sum a[i] b[i], i < n; dev_a may equal dev_b.  n = 0 gives zero. */
int mnt753_vec_dot(int curve, const uint64_t* dev_a, const uint64_t* dev_b, size_t n, uint64_t* host_out, void* stream);
/* sum c[i] t^i, i < n; t canonical (else MNT753_EINVAL); host result as above. */
int mnt753_poly_eval(int curve, const uint64_t* dev_coeffs, size_t n, const uint64_t* host_t, uint64_t* host_out, void* stream);
/* the values at t of the k <= 3 polynomials of degree < m that take dev_vecs[j][i] at the domain's i-th element, every kind of
 * domain, t anywhere (inside the domain it returns that element of each vector).  dev_u: m elements of scratch, receives L(t)
 * (the words of mnt753_domain_lagrange_at, whose workspace and ordering rules apply). */
int mnt753_domain_interp_at(mnt753_domain* d, const uint64_t* host_t, const uint64_t* const* dev_vecs, int k, uint64_t* dev_u,
                            uint64_t* host_out /* k elements */, void* stream);
typedef struct { int32_t ok, reserved; uint64_t lhs[12], rhs[12]; } mnt753_h_check_result;   /* A(t)B(t) - C(t) and Z(t)H(t) */
/* after compute_h: host_abc = A(t) | B(t) | C(t) from mnt753_domain_interp_at BEFORE compute_h overwrote the vectors; dev_h the m + 1
 * coefficients.  A failed identity is ok = 0 with return code 0; with probability >= 1 - 2m/r over t it fails whenever a row has
 * ca cb != cc or a coefficient of H is wrong.  t inside the domain (Z(t) = 0, the check would say nothing about H) is MNT753_EINVAL,
 * as in mnt753_groth16_generate; so are t >= r and a non-canonical host_abc.  An error leaves *out untouched. */
int mnt753_h_check(mnt753_domain* d, const uint64_t* host_t, const uint64_t* host_abc, const uint64_t* dev_h, mnt753_h_check_result* out,
                   void* stream);
/* interp_at (k = 3) + mnt753_compute_h + mnt753_h_check.  host_t == NULL: t from getrandom, reduced below r, redrawn if inside the
 * domain.  No workspace beyond mnt753_domain_lagrange_at's: L(t) lies in dev_h until compute_h writes there.  A refused t leaves the
 * vectors, dev_h and *out untouched. */
int mnt753_compute_h_checked(mnt753_domain* d, uint64_t* dev_ca, uint64_t* dev_cb, uint64_t* dev_cc, uint64_t* dev_h, const uint64_t* host_t,
                             mnt753_h_check_result* out, void* stream);

/* ---- witness-map front end (the step before the hot path) -------------------------------------------
 * The reference evaluates the constraint system on the assignment on the CPU before the prover starts
 * (libsnark/generate_parameters.cpp:44-57 writes the result into the input file as ca / cb / cc; it is the first loop of
 * r1cs_to_qap_witness_map, libsnark/reductions/r1cs_to_qap/r1cs_to_qap.tcc:223-237).  Here the constraint system lives on the
 * device as three CSR matrices (a, b, c) over the variables (1, w_1 .. w_m) -- column 0 is the constant one, i.e. w[0] of the
 * input file -- and the evaluation is one kernel:
 *   ca[i] = <a_i, w>, cb[i] = <b_i, w>, cc[i] = <c_i, w> for i < nc;  ca[nc + i] = w[i] for i <= num_inputs;  zero above.
 * row_ptr[k]: nc + 1 offsets (row_ptr[k][0] = 0), col[k]: variable indices 0 .. m, coeff[k]: Fr elements in wire form;
 * host pointers.  out_len = the evaluation domain size (d + 1 >= nc + num_inputs + 1). */
typedef struct mnt753_r1cs mnt753_r1cs;
int mnt753_r1cs_create(int curve, uint64_t num_inputs, uint64_t m, uint64_t nc, const uint64_t* const row_ptr[3], const uint32_t* const col[3],
                       const uint64_t* const coeff[3], mnt753_r1cs** out);
int mnt753_r1cs_free(mnt753_r1cs* r);
size_t mnt753_r1cs_domain_size(const mnt753_r1cs* r);   /* nc + num_inputs + 1 */
size_t mnt753_r1cs_num_variables(const mnt753_r1cs* r); /* m: dev_w of mnt753_r1cs_evaluate must hold m + 1 elements */
size_t mnt753_r1cs_num_inputs(const mnt753_r1cs* r);
int mnt753_r1cs_evaluate(mnt753_r1cs* r, const uint64_t* dev_w, uint64_t* dev_ca, uint64_t* dev_cb, uint64_t* dev_cc, size_t out_len, void* stream);
/* The instance map with evaluation: replaces r1cs_to_qap_instance_map_with_evaluation (libsnark/reductions/r1cs_to_qap/r1cs_to_qap.tcc:
 * 105-175), the call every libsnark generator starts with (r1cs_gg_ppzksnark.tcc:223).  With u = the Lagrange coefficients of d at t:
 *   At[i] = u[nc + i] for i <= num_inputs;  every term (row, col, coeff) of a / b / c adds u[row] coeff to At / Bt / Ct[col];
 *   Ht[i] = t^i for i <= m_d = mnt753_domain_size(d);  Zt = Z(t).
 * dev_At / dev_Bt / dev_Ct: num_variables + 1 elements each, dev_Ht: m_d + 1, host_Zt: one element in host memory (written before the
 * call returns; the device vectors are complete when `stream` has run).  MNT753_EINVAL, with nothing enqueued and nothing written: a
 * null pointer, a domain of the other curve or on another device, m_d < nc + num_inputs + 1, t >= r.
 * The sums go by column and the matrices lie by row: the first call on a system builds a column-major view of it (a permutation of
 * 8 bytes per term, on the host, from the index arrays copied back from the device) and keeps it until mnt753_r1cs_free;
 * mnt753_r1cs_create and the prover path pay nothing for it.  Every column is cut into chunks of at most chunk_terms terms, one device
 * thread each, so that a column holding a large share of all terms (the constant, column 0) does not serialise behind one lane.
 * The partial sums and the copy of u belong to the system and are shared by its calls: calls on different streams are ordered on the
 * device one after the other (an event per system, as for a domain's work buffer), and host threads must not enter the same system
 * at the same time.  The system lives on the device that was current when it was created and the call runs there; a domain on
 * another device is MNT753_EINVAL. */
typedef struct {
  uint32_t chunk_terms, reserved;   /* L: terms per chunk at most */
  uint64_t terms;                   /* terms of a, b and c together */
  uint64_t work_items;              /* chunks = threads of the column-sum kernel */
  uint64_t split_columns;           /* columns cut into more than one chunk */
  uint64_t longest_column;          /* terms of the longest column */
  uint64_t transpose_bytes;         /* device memory of the column-major view (permutation, chunk and work lists) */
  uint64_t partial_bytes;           /* device memory of the partial sums, 112 bytes per chunk */
} mnt753_qap_plan;
/* the plan of a system; builds the column-major view if no call has yet */
int mnt753_r1cs_qap_plan(const mnt753_r1cs* r, mnt753_qap_plan* out);
int mnt753_r1cs_qap_at(mnt753_r1cs* r, mnt753_domain* d, const uint64_t* host_t, uint64_t* dev_At, uint64_t* dev_Bt, uint64_t* dev_Ct,
                       uint64_t* dev_Ht, uint64_t* host_Zt, void* stream);

/* ---- Groth16 key generation from given randomness -----------------------------------------------------
 * swap_AB_if_beneficial (libsnark/relations/constraint_satisfaction_problems/r1cs/r1cs.tcc:194-243): counts the variables (columns
 * 0 .. m) that a term of a and a term of b touch; if b touches STRICTLY more, a and b change roles inside the system object: the
 * matrices' device arrays change places and the row work list is renumbered in place, no matrix is copied (a column-major view that
 * an earlier mnt753_r1cs_qap_at built is dropped and rebuilt by the next one).  *swapped (may be NULL) = 1 if this call exchanged them.
 * The prover must evaluate the system as it now stands: mnt753_r1cs_evaluate and mnt753_r1cs_qap_at do.  The count reads the column
 * indices back from the device (4 bytes per term of a and b) and runs on the host; the call blocks. */
int mnt753_r1cs_swap_ab_if_beneficial(mnt753_r1cs* r, int* swapped);
/* 1 if a and b stand exchanged relative to the arrays mnt753_r1cs_create was given (an odd number of swaps), else 0 */
int mnt753_r1cs_is_swapped(const mnt753_r1cs* r);

/* Stable compaction of the non-zero elements of a device vector of n < 2^32 Fr elements (all 12 words zero = zero): dev_compact
 * receives the non-zero elements in their order, dev_index their strictly increasing original indices, *host_count their number --
 * the "query density" of r1cs_gg_ppzksnark.tcc:230-244 when the vector is At or Bt.  Three kernels (csrc/keygen_kernels.hip.h): per
 * workgroup the flags and their count by wave ballots, one workgroup scanning the counts, and the write at ballot-prefix positions;
 * no atomics, the same output whatever the scheduling.  dev_compact / dev_index may both be NULL: only the count is taken.  Room for n
 * entries each.  Blocks until *host_count is written.  n = 0: count 0, nothing launched. */
int mnt753_compact_nonzero(const uint64_t* dev_scalars, size_t n, uint64_t* dev_compact, uint32_t* dev_index, size_t* host_count, void* stream);
/* dev_out[dev_index[j]] = dev_rows[j] for j < count, rows of row_words u64, and zero words in every other of the n rows of dev_out. */
int mnt753_scatter_rows(const uint64_t* dev_rows, const uint32_t* dev_index, size_t count, size_t row_words, uint64_t* dev_out, size_t n, void* stream);
/* mnt753_batch_exp for a vector with many zeros (kc_batch_exp works on a sparse vector for the same reason, knowledge_commitment/
 * kc_multiexp.tcc): the non-zero scalars are compacted, walked, and their rows scattered back; a zero scalar costs no walk.  The
 * same words as mnt753_batch_exp writes, everywhere.  Both ends on the device.  *host_count (may be NULL) = non-zero scalars.
 * count == 0 launches no walk (the output is zeroed); count == n is the plain mnt753_batch_exp on the vector as it lies.  Unlike
 * mnt753_batch_exp the call allocates its compacted vectors (100 bytes per scalar and one output row per non-zero scalar), blocks on
 * the count, and returns when the output is complete. */
int mnt753_batch_exp_sparse(mnt753_fixed_base* fb, const uint64_t* dev_scalars, size_t n, const uint64_t* host_coeff, uint64_t* dev_out_affine,
                            size_t* host_count, void* stream);
/* dev_out[i] = (beta At[i] + alpha Bt[i] + Ct[i]) c_i, i < n, c_i = 1 for i <= num_inputs and dinv above: entries 0 .. num_inputs are
 * the ABC of r1cs_gg_ppzksnark.tcc:257-261, the rest is Lt (:266-273, dinv = delta^-1).  One fused kernel, wire form in and out; beta,
 * alpha, dinv: canonical Fr elements in HOST memory.  dev_out may be one of the inputs. */
int mnt753_keygen_combine(int curve, const uint64_t* dev_At, const uint64_t* dev_Bt, const uint64_t* dev_Ct, size_t n, size_t num_inputs,
                          const uint64_t* host_beta, const uint64_t* host_alpha, const uint64_t* host_dinv, uint64_t* dev_out, void* stream);

/* r1cs_gg_ppzksnark_generator (libsnark/zk_proof_systems/ppzksnark/r1cs_gg_ppzksnark/r1cs_gg_ppzksnark.tcc:212-362) with its
 * randomness -- t, alpha, beta, delta (:216-219) and the G1 generator (:290) -- turned into arguments: a key is a pure function of
 * (constraint system, randomness).  The G2 generator is G2::one() (:300), a constant of the library.
 * mnt753_keygen_sizes: elements of each output for a system and a domain of m_d elements (r1cs_gg_ppzksnark.tcc:281, :318-352;
 * the challenge's parameter file writes them in this order, generate_parameters.cpp:60-85). */
typedef struct {
  uint64_t a_query;      /* m + 1 G1 */
  uint64_t b_g1_query;   /* m + 1 G1 */
  uint64_t b_g2_query;   /* m + 1 G2 */
  uint64_t l_query;      /* m - num_inputs G1 */
  uint64_t h_query;      /* m_d - 1 G1 */
  uint64_t abc_g1;       /* num_inputs + 1 G1 */
} mnt753_keygen_sizes;
int mnt753_groth16_sizes(const mnt753_r1cs* r, const mnt753_domain* d, mnt753_keygen_sizes* out);
/* where a key goes: the query vectors on the device (affine wire format, the identity as all-zero words -- write_g1 / write_g2 of
 * libsnark/serialization.hpp:44-67 -- sized by mnt753_keygen_sizes; each can go straight into mnt753_bases_create(.., on_device = 1, ..)),
 * the five single elements in host memory (24 words G1, mnt753_affine_words(curve, MNT753_G2) words G2). */
typedef struct {
  uint64_t *dev_a_query, *dev_b_g1_query, *dev_b_g2_query, *dev_l_query, *dev_h_query, *dev_abc_g1;
  uint64_t *host_alpha_g1, *host_beta_g1, *host_beta_g2, *host_delta_g1, *host_delta_g2;
} mnt753_keygen_out;
/* Window widths and tiles of the two mnt753_fixed_base objects of a call (0 = the library's default, as for mnt753_fixed_base_create)
 * and whether a query goes through mnt753_batch_exp_sparse.  By default the queries of At and Bt do, in G1 and in G2 (measured:
 * DESIGN.md section 4.11 has the figures and the rule); MNT753_KEYGEN_DENSE_G1 / MNT753_KEYGEN_DENSE_G2 walk those vectors as they
 * lie.  ABC | Lt and Ht always do (Ht has no zero entry, Lt is zero only where a variable is in no constraint).  Arguments of the
 * call: there is no environment variable and no process-wide setting. */
#define MNT753_KEYGEN_DENSE_G1 1u
#define MNT753_KEYGEN_DENSE_G2 2u
typedef struct {
  int g1_window_bits, g2_window_bits;
  size_t g1_tile, g2_tile;
  unsigned flags, reserved;
} mnt753_keygen_opts;
typedef struct {
  uint64_t non_zero_at, non_zero_bt;   /* the query densities of r1cs_gg_ppzksnark.tcc:230-244 */
  int swapped;                         /* 1 if this call's swap_AB_if_beneficial exchanged a and b */
  int reserved;
} mnt753_keygen_report;
/* The steps: mnt753_r1cs_swap_ab_if_beneficial (:213; the system object STAYS swapped -- the prover must evaluate the swapped system,
 * so report->swapped tells), mnt753_r1cs_qap_at (:223), the densities (:230-244), mnt753_keygen_combine (:252-274), Ht cut by two
 * (:281), the G1 and G2 window tables (:289-307), the five single elements through mnt753_point_scale (:310-314), and mnt753_batch_exp
 * for At, Bt (G1 and G2), Ht with the coefficient Zt delta^-1, Lt and ABC (:318-352; ABC_0 goes with the rest of ABC through the
 * table, the same point).  d: a domain of at least nc + num_inputs + 1 elements, any kind mnt753_r1cs_qap_at accepts.  opts may be NULL
 * (all zero).  The call allocates its tables and vectors, blocks, and returns when every output is complete.
 * MNT753_EINVAL with nothing enqueued for the key, the system left as it was and no output written -- each a DELIBERATE departure from
 * the reference, which goes on and writes a useless key (delta = 0 even divides by zero: Fp_model::invert of 0):
 *   - alpha, beta or delta is zero, or one of t, alpha, beta, delta is >= r;
 *   - Z(t) = 0, i.e. t lies in the domain (every H entry would be the identity);
 *   - the G1 generator is the identity or fails mnt753_check_points (that one check kernel does run);
 * and, as for mnt753_r1cs_qap_at: a null pointer, a domain that is too small, of the other curve or on another device.
 * The GT element alpha_g1_beta_g2 of a libsnark verification key (:348) is a pairing of two of the outputs: mnt753_vk_create below
 * computes it from alpha_g1 and beta_g2 and mnt753_vk_serialize writes the complete key (`main_hip <curve> vk`). */
int mnt753_groth16_generate(mnt753_r1cs* r, mnt753_domain* d, const uint64_t* host_t, const uint64_t* host_alpha, const uint64_t* host_beta,
                            const uint64_t* host_delta, const uint64_t* host_g1_generator, const mnt753_keygen_opts* opts,
                            const mnt753_keygen_out* out, mnt753_keygen_report* report, void* stream);
/* G1::one() / G2::one() of the curve in the affine wire format (mnt4753_init.cpp:140-142, :201-203; mnt6753_init.cpp:150-155, :213-219):
 * the G2 generator mnt753_groth16_generate uses, and the G1 generator `main_hip generate` takes when no randomness file names one. */
int mnt753_group_generator(int curve, int group, uint64_t* out_affine);

/* ---- the pairing and Groth16 verification -------------------------------------------------------------
 * The reduced flipped ate pairing of the curve: replaces libff's mnt{4,6}753_ate_reduced_pairing (depends/libff/libff/algebra/curves/
 * mnt753/mnt4753/mnt4753_pairing.cpp:681-688: ate_precompute_G1 / _G2, ate_miller_loop, final_exponentiation), for a batch.
 * GT element: an element of Fq4 = Fq2[v]/(v^2 - u) (MNT4753) or Fq6 = Fq3[v]/(v^2 - u) (MNT6753) as c0 | c1, each an Fq2 / Fq3 element
 * in the wire form of a G2 coordinate: mnt753_gt_words(curve) = 48 / 72 words, what operator<< writes under BINARY_OUTPUT and
 * MONTGOMERY_OUTPUT. */
size_t mnt753_gt_words(int curve);
/* out_gt[i] = e(g1_affine[i], g2_affine[i]) for i < n: affine wire-format points; on_device != 0: the three pointers are device
 * pointers.  One lane group (2 or 3 lanes) per pairing; the call blocks until out_gt is complete.  Both arguments go through
 * mnt753_check_points first: a non-canonical coordinate or a point off its curve is MNT753_EINPUT and nothing is computed (no
 * subgroup test for G2: not checked unless the caller runs mnt753_check_subgroup first).  The identity in either argument gives GT
 * one -- a DELIBERATE departure from libff, whose precomputation runs on the identity's coordinates and returns a value without
 * meaning. */
int mnt753_pairing(int curve, const uint64_t* g1_affine, const uint64_t* g2_affine, size_t n, int on_device, uint64_t* out_gt, void* stream);
/* A Groth16 verification key on the device: the counterpart of libsnark's r1cs_gg_ppzksnark_verifier_process_vk
 * (r1cs_gg_ppzksnark.tcc:499-512).  alpha_g1, beta_g2, delta_g2, abc_g1 (num_inputs + 1 points): affine wire form in host memory --
 * the contents of `generate`'s vk_elements.bin.  Computes e(alpha_g1, beta_g2) on the device and keeps delta_g2, G2::one() and ABC
 * there, and -- as libsnark's precompute_G2 does for vk_generator_g2_precomp and vk_delta_g2_precomp -- the Miller-loop coefficients of
 * G2::one() and delta_g2 (H, 4C, J, L of every doubling step, L1, RZ of every addition step: mnt753_vk_coefficient_bytes, 0.83 MB on
 * MNT4753 and 1.25 MB on MNT6753 for both points), computed once by one lane group each; every proof's lane group reads them from the
 * key.  MNT753_EINVAL: an element is the identity; MNT753_EINPUT: an element is non-canonical or off its curve.  The key lives on the
 * device that is current when it is created. */
typedef struct mnt753_vk mnt753_vk;
int mnt753_vk_create(int curve, const uint64_t* alpha_g1, const uint64_t* beta_g2, const uint64_t* delta_g2, const uint64_t* abc_g1, size_t num_inputs,
                     mnt753_vk** out);
int mnt753_vk_destroy(mnt753_vk* vk);
size_t mnt753_vk_num_inputs(const mnt753_vk* vk);
size_t mnt753_vk_coefficient_bytes(const mnt753_vk* vk);   /* device memory of the stored coefficients of the key's two G2 points */
/* The device memory a mnt753_groth16_verify call on this key may allocate for a chunk of proofs, in bytes: the batch runs in chunks of
 * cap / (194 + 96 num_inputs) proofs (host-memory batches: 8 proof words + 96 num_inputs more per proof for the staged copy), at
 * least one and at most 2^16.  0 (the default): chunks of 2^16 proofs.  mnt753_groth16_verify_folded_locate runs chunks of WHOLE
 * segments (128 / 84 proofs), at least one segment, after what it keeps per segment of the call has come off the cap: (cap - segments
 * per_segment) / (g per_proof) segments per chunk, per_proof = 546 (+ 96 (num_inputs + 1) with public inputs, + the staged copy of a
 * host batch), per_segment = 516 + g + 96 (num_inputs + 1) + one GT element in device form (448 / 672 bytes) (+ 336 (slices + 1) + 112
 * with a prepared key); see that call's comment. */
int mnt753_vk_set_workspace_cap(mnt753_vk* vk, size_t bytes);
/* alpha_g1_beta_g2 of the key, mnt753_gt_words words */
int mnt753_vk_gt(const mnt753_vk* vk, uint64_t* out);
/* The bytes the reference writes for r1cs_gg_ppzksnark_verification_key (operator<<, r1cs_gg_ppzksnark.tcc:99-106) when built with
 * BINARY_OUTPUT, MONTGOMERY_OUTPUT and NO_PT_COMPRESSION: GT | '0' delta_g2 | '0' ABC_g1[0] | the sparse_vector of the rest (domain
 * size, number of indices, the indices, number of values, each followed by a newline, then '0' ABC_g1[j] for j >= 1).  *len = the
 * size; buf == NULL asks for the size alone, cap < *len is MNT753_EINVAL. */
int mnt753_vk_serialize(const mnt753_vk* vk, uint8_t* buf, size_t cap, size_t* len);
/* out_affine[i] = ABC_g1[0] + sum_j inputs[i][j] ABC_g1[j + 1] for i < n (inputs: n x num_inputs Fr, host memory; out: n G1 points,
 * affine wire form, the identity as zero words): the accumulation of r1cs_gg_ppzksnark_online_verifier_weak_IC (:522-525).  One lane
 * per proof, a joint double-and-add over the bits of its inputs: 753 doublings and on average 753 num_inputs / 2 additions in that
 * lane: right for a handful of public inputs.  A key with more of them is prepared once (mnt753_vk_prepare_inputs below) and this call,
 * like the verifiers, then walks window tables -- the same words in out_affine.  MNT753_EINPUT: an input is >= r. */
int mnt753_vk_accumulate(const mnt753_vk* vk, const uint64_t* inputs, size_t n, uint64_t* out_affine);
/* ---- input tables of a key: public inputs by the fixed-base method ------------------------------------
 * The ABC points of a key are fixed bases, so the accumulation of r1cs_gg_ppzksnark_online_verifier_weak_IC (r1cs_gg_ppzksnark.tcc:
 * 522-525) can run as libff's get_window_table / windowed_exp / batch_exp (depends/libff/libff/algebra/scalar_multiplication/
 * multiexp.tcc:547-720) with one table per ABC point: W = ceil(754 / w) mixed additions per input instead of 753 doublings and some
 * 376 additions.  An opt-in property of the key OBJECT: nothing prepares a key by itself, no environment variable or process-wide
 * setting is read, and a key that was not prepared launches exactly what it launched before.
 * mnt753_vk_prepare_inputs builds one signed-digit window table (the layout of mnt753_fixed_base_create: multiples 1 .. 2^(w-1) of
 * 2^(jw) ABC[p] for every window j, 256-byte affine rows) per ABC point, ABC[0] included, in ONE allocation owned by the key:
 * (num_inputs + 1) W 2^(w-1) 256 bytes.  window_bits = 0: the widest w in 2 .. 16 whose tables fit max_table_bytes
 * (0: 256 MiB, the Infinity Cache of the MI355X).  MNT753_EINVAL, with the key left as it was and a message that names the bytes
 * needed and the cap: an explicit width that does not fit, w = 2 not fitting, window_bits outside 2 .. 16 (other than 0), a key
 * without inputs.  Calling it again replaces the tables; mnt753_vk_release_inputs frees them and returns the key to the unprepared
 * path; mnt753_vk_destroy frees them too.  mnt753_vk_coefficient_bytes keeps its meaning: the tables are reported by the plan only.
 * The build is O(w) launches per 2^17 rows of a level, not a loop over the inputs.
 * A prepared key takes the table path in mnt753_vk_accumulate, mnt753_groth16_verify, _verify_ex, _verify_compressed and
 * _verify_folded: per chunk one lane per (proof, slice of inputs_per_lane consecutive inputs) walks its inputs' digits, one lane
 * per proof sums ABC[0] and the proof's partial sums, and the accumulated points reach the pairing kernel word for word as
 * k_vk_accumulate writes them -- verdicts, status bytes and the identity / input >= r cases are unchanged.  inputs_per_lane is chosen
 * per chunk: as many slices as bring the chunk to 65536 lanes, one input per lane for a single proof, one lane per proof from 65536
 * proofs on.  Workspace per proof of a chunk, beside what mnt753_vk_set_workspace_cap's comment lists: 336 (slices + 1) + 112
 * bytes, slices = ceil(num_inputs / inputs_per_lane); the chunk is cap / (194 + 96 num_inputs + 336 (slices + 1) + 112) proofs, with
 * inputs_per_lane chosen for the chunk that runs (a cap that shrinks the chunk gives its proofs more slices, settled in a few rounds).
 * The fold with a prepared key: c_j for all inputs of a chunk from one launch over the columns (no gather, no host round trip per
 * input), and S = rho ABC[0] + sum_j c_j ABC[j + 1] on the device as ONE walk over num_inputs + 1 scalars, ABC[0]'s table in place
 * of the implicit 1.
 * mnt753_vk_input_plan fills *out for a chunk of n proofs (n = 0 counts as 1): prepared = 0 and zeros for a key without tables. */
typedef struct { int window_bits, windows; uint32_t inputs_per_lane; uint32_t reserved; uint64_t table_bytes; int prepared; int reserved2; } mnt753_vk_input_plan_t;
int mnt753_vk_prepare_inputs(mnt753_vk* vk, int window_bits /* 0 = default */, size_t max_table_bytes /* 0 = 256 MiB */);
int mnt753_vk_input_plan(const mnt753_vk* vk, size_t n /* proofs of a chunk, for inputs_per_lane */, mnt753_vk_input_plan_t* out);
int mnt753_vk_release_inputs(mnt753_vk* vk);
/* Verifies n proofs against the key: r1cs_gg_ppzksnark_online_verifier_weak_IC (:515-567) per proof, one lane group each.
 * proofs: n x (A | B | C), affine wire form, the layout `complete` writes; inputs: n x num_inputs Fr (without the leading 1);
 * on_device != 0: both are device pointers.  verdicts (host memory, n bytes): 0 accepted, 1 malformed, 2 the pairing check failed.
 * Malformed: a non-canonical coordinate, a point off its curve, the identity as A, B, C or as the accumulated input point, an input
 * >= r; such a proof runs the arithmetic on stand-in points, its neighbours in the wave are not disturbed.  The check is
 * FE(ML(A, B) ML(-acc, G2::one()) ML(-C, delta_g2)) == alpha_g1_beta_g2: one Miller loop over three pairs and one final
 * exponentiation; the same verdict as the reference's form (:409-414), from which it differs by a factor the final exponentiation
 * maps to one.  Subgroup membership of B is NOT checked, as in the reference, unless mnt753_groth16_verify_ex is called with
 * MNT753_VERIFY_CHECK_SUBGROUP (DESIGN.md sections 4.13 and 8).  Returns the number of proofs not
 * accepted (>= 0), or a negative MNT753_E* code.  The batch runs in chunks under mnt753_vk_set_workspace_cap (by default 2^16 proofs:
 * at most 2^16 (194 + 96 num_inputs) bytes, plus the staged copy of a chunk that arrives in host memory); one allocation of each
 * buffer per call.  With on_device, proofs and inputs must lie on the key's device (MNT753_EINVAL otherwise).  Only B is stepped
 * through the Miller loop; the coefficients of G2::one() and delta_g2 are read from the key.  Blocks until verdicts is complete. */
int mnt753_groth16_verify(const mnt753_vk* vk, const uint64_t* proofs, const uint64_t* inputs, size_t n, int on_device, uint8_t* verdicts, void* stream);
/* mnt753_groth16_verify with options.  flags == 0 is mnt753_groth16_verify itself (which is a call of this one and never returns
 * verdict 3); an unknown bit is MNT753_EINVAL.  MNT753_VERIFY_CHECK_SUBGROUP: B of every proof is also tested for membership in G2, the
 * order-r subgroup of the twist -- psi(B) == [t - 1] B on the running point the Miller loop holds anyway, an
 * exact test per proof -- and a well-formed proof whose B fails it gets verdict 3, "B is not in the subgroup".  Precedence: malformed
 * (1), then 3, then the pairing check (2).  The key's own beta_g2 and delta_g2 are NOT tested by this call or by mnt753_vk_create:
 * mnt753_check_subgroup does that. */
#define MNT753_VERIFY_CHECK_SUBGROUP 1u
int mnt753_groth16_verify_ex(const mnt753_vk* vk, const uint64_t* proofs, const uint64_t* inputs, size_t n, int on_device, unsigned flags, uint8_t* verdicts,
                             void* stream);
/* Randomised batch verification: the n proofs folded into ONE final exponentiation.  An opt-in beside the
 * exact calls above, with a different soundness statement.  proofs, inputs, on_device, stream and the chunking under
 * mnt753_vk_set_workspace_cap as for mnt753_groth16_verify.  coefficients: n x 2 words in HOST memory, rho_i = word 0 + 2^64 word 1,
 * 0 < rho_i < 2^128; they are an ARGUMENT, as the randomness of mnt753_groth16_generate is: the library draws nothing.  With
 *     U_i = rho_i A_i,  T = sum rho_i C_i,  rho = sum rho_i,  c_j = sum_i rho_i x_ij mod r,  S = rho ABC[0] + sum_j c_j ABC[j + 1]
 * the batch is accepted iff  FE( prod_i ML(U_i, B_i) ML(-S, G2::one()) ML(-T, delta_g2) ) == alpha_g1_beta_g2^rho:  per proof one
 * stepped Miller loop with ONE line value per step and two 128-bit scalar multiplications in G1; the two stored pairs of the key, the
 * final exponentiation and the power of alpha_g1_beta_g2 once per call.
 * Soundness.  Let every A_i and C_i lie on its curve (G1 has cofactor 1), every B_i lie in G2, and beta_g2 and delta_g2 of the key lie
 * in G2.  Then each proof's defect d_i = e(A_i, B_i) e(acc_i, G2::one())^-1 e(C_i, delta_g2)^-1 e(alpha_g1, beta_g2)^-1 lies in the
 * order-r subgroup of GT and the check is prod d_i^rho_i == 1: if some d_i != 1 and the rho_i are drawn uniformly AFTER the proofs are
 * fixed, it passes with probability at most 1 / (2^128 - 1).  Coefficients an adversary can predict prove nothing (two defects can
 * cancel).  The curve checks of A, B, C and the subgroup test of every B_i (psi(B) == [t - 1] B on the running point of its Miller
 * loop) are therefore part of THIS call, not a flag; beta_g2 and delta_g2 of the key remain the caller's duty (mnt753_check_subgroup),
 * as for mnt753_groth16_verify_ex.
 * status (host memory, n bytes, may be NULL): per proof 0, 1 (malformed, as for mnt753_groth16_verify) or 3 (B is not in the
 * subgroup); there is no per-proof 2.  One difference from the per-proof verifier: acc_i is never formed, so "acc_i is the identity"
 * is not reported as malformed (meeting that case needs a discrete-logarithm relation among the ABC points).
 * *accepted = 1 iff every status byte is 0 and the folded equation holds; a rejected batch does not say WHICH proof is wrong: run
 * mnt753_groth16_verify_ex with MNT753_VERIFY_CHECK_SUBGROUP to name it.  n = 0: *accepted = 1.  Returns 0, or a negative code:
 * MNT753_EINVAL for a null pointer, a zero coefficient, n > 2^24 or memory on another device.  Workspace per proof of a chunk:
 * 546 bytes, with public inputs 96 (num_inputs + 1) more, plus its staged copy if it arrives in host memory, and one GT element per
 * 128 (MNT6753: 84) proofs.  Blocks until the verdict is there. */
int mnt753_groth16_verify_folded(const mnt753_vk* vk, const uint64_t* proofs, const uint64_t* inputs, size_t n, int on_device,
                                 const uint64_t* coefficients /* n x 2 words, host */, uint8_t* status /* n, host, may be NULL */, int* accepted, void* stream);
/* The fold that names the wrong proofs: one tail per SEGMENT.  A segment is one workgroup of the fold's Miller
 * kernel: mnt753_fold_segment_proofs(curve) = 128 (MNT4753) or 84 (MNT6753) consecutive proofs, segment s holding the proofs
 * [s g, min(n, (s + 1) g)); 0 for an unknown curve.  With the rho_i of the caller as for mnt753_groth16_verify_folded, segment s has
 *     F_s = prod ML(rho_i A_i, B_i),  T_s = sum rho_i C_i,  rho_s = sum rho_i (< 2^135),  c_js = sum rho_i x_ij mod r,
 *     S_s = rho_s ABC[0] + sum_j c_js ABC[j + 1]        (products and sums over the proofs i of the segment)
 * and is accepted iff none of its proofs has a status (1 or 3) and FE(F_s ML(-S_s, G2::one()) ML(-T_s, delta_g2)) ==
 * alpha_g1_beta_g2^rho_s: the equation and the soundness statement of mnt753_groth16_verify_folded on the segment, 2^-128 per segment
 * and a union bound over the segments of a call.  There is no global F, T or tail: all segment tails of a call run side by side in one launch, one
 * lane group each.  A segment that is not accepted is handed WHOLE to the per-proof verifier, mnt753_groth16_verify_ex with
 * MNT753_VERIFY_CHECK_SUBGROUP (adjacent rejected segments as one range), and its proofs get that verifier's bytes; the proofs of an
 * accepted segment get 0.
 * verdicts (host memory, n bytes, REQUIRED): 0, 1, 2, 3 as for mnt753_groth16_verify_ex.  Returns the number of proofs not accepted
 * (>= 0) or a negative code, as mnt753_groth16_verify does; n = 0 returns 0.  Arguments, device rules and errors are those of
 * mnt753_groth16_verify_folded: MNT753_EINVAL for a null pointer, a zero coefficient, n > 2^24 or memory on another device.
 * Two things to know.  (1) The one semantic difference inherited from the fold: inside an ACCEPTED segment acc_i is never formed, so
 * "acc_i is the identity" is not reported there (a rechecked segment reports it, as the per-proof verifier does).  (2) A segment that
 * contains a proof with a status is rechecked whole; the flagged proof is not masked out of rho_s and c_js, so its neighbours in the
 * segment pay the per-proof pass as well.
 * Chunks: a chunk is a whole number of segments and at least one, at most 2^16 proofs rounded down to whole segments.  The scaling,
 * the point sums, the Miller loops and the segment scalars run per chunk; what they leave per SEGMENT is kept for the whole call, and
 * S_s and the tails of ALL segments of the call then run in one launch each.  Under mnt753_vk_set_workspace_cap a proof of a chunk
 * takes 546 bytes (with public inputs 96 (num_inputs + 1) more, plus its staged copy if it arrives in host memory); a segment of the
 * CALL takes one GT element in device form (448 / 672 bytes), 192 + 192 bytes for S_s and T_s, 32 + 96 for rho_s, 4 for its verdict,
 * 128 / 84 status bytes, 96 (num_inputs + 1) for the scalars of S_s, and with a prepared key the 336 (slices + 1) + 112 bytes of its
 * walk.  The segments' share comes off the cap first, the rest bounds the chunk; a cap below that still runs one segment per chunk.
 * The recheck allocates as mnt753_groth16_verify_ex does, under the same cap, before the fold's buffers are freed.  Rejected segments
 * that are not all adjacent are gathered into ONE batch for it (a copy of their proofs and inputs, 8 proof words + 96 num_inputs bytes
 * per rechecked proof, on the device for a device batch and in host memory for a host batch): a call of the per-proof verifier is one
 * serial chain deep whatever its size.  Where a cap is set and that copy would exceed it, every run is verified where it lies instead.
 * report (may be NULL): the segments of the call, how many were rejected, how many proofs the per-proof verifier rechecked, and the
 * milliseconds on the device of the scaling with the point sums, the Miller loops, the segment scalars / S_s / tails, and (host clock)
 * of the recheck.  Blocks until verdicts is complete. */
size_t mnt753_fold_segment_proofs(int curve);
typedef struct { uint64_t segments, segments_rejected, proofs_rechecked; float ms_scale, ms_miller, ms_tails, ms_recheck; } mnt753_fold_locate_report;
int mnt753_groth16_verify_folded_locate(const mnt753_vk* vk, const uint64_t* proofs, const uint64_t* inputs, size_t n, int on_device,
                                        const uint64_t* coefficients /* n x 2 words, host */, uint8_t* verdicts /* n, host, required */,
                                        mnt753_fold_locate_report* report /* may be NULL */, void* stream);

/* ---- input validation (device) --------------------------------------------------------------------------
 * The reference prover trusts its files (unchecked fread, prover_reference_functions.cpp:48-116); what the reference HAS for the
 * purpose is libff's G::is_well_formed() (depends/libff/libff/algebra/curves/mnt753/mnt4753/mnt4753_g1.cpp:348, mnt4753_g2.cpp:371-396,
 * mnt6753_g1.cpp:348, mnt6753_g2.cpp:377: the curve equation) and r1cs_constraint_system::is_satisfied, asserted before a witness is
 * mapped (libsnark/reductions/r1cs_to_qap/r1cs_to_qap.tcc:216).  These calls are those checks on wire-format words, on the device
 * (csrc/mnt753_validate.hip).  A malformed input is a RESULT, not a failed call: they return 0 and fill *out (host memory; the call
 * blocks until it is filled) with the number of bad elements, the lowest bad index and that index's reason -- the same record
 * whatever the scheduling.  n = 0 gives an all-zero report.  Null pointers / bad ids: MNT753_EINVAL; no device: MNT753_ENODEV.
 * MNT753_EINPUT is what the wrapper classes and main_hip make of a report with n_bad > 0 (main_hip: exit code 3). */
#define MNT753_EINPUT (-7)            /* an input failed validation (wrapper / CLI level; the check calls themselves return 0) */
enum { MNT753_BAD_NONE = 0, MNT753_BAD_NONCANONICAL = 1, MNT753_BAD_OFF_CURVE = 2, MNT753_BAD_UNSATISFIED = 3, MNT753_BAD_NOT_IN_SUBGROUP = 4 };
typedef struct { uint64_t n_bad, first_bad; uint32_t first_reason, reserved; } mnt753_check_report;
/* n affine points in the wire format (on_device != 0: a device pointer).  Per point, the first that applies: a coordinate component
 * >= q -> MNT753_BAD_NONCANONICAL; all words of y zero -> the identity as read_g1 / read_g2 decode it (serialization.hpp:84-111),
 * well formed whatever x holds; y^2 != x^3 + a x + b (G2: the twist's a', b', mnt4753_init.cpp:122-123, mnt6753_init.cpp:133-136) ->
 * MNT753_BAD_OFF_CURVE.  is_well_formed() of the four groups; like it, no subgroup test for G2: that is not checked unless
 * mnt753_check_subgroup is called (DESIGN.md sections 4.13 and 8). */
int mnt753_check_points(int curve, int group, const uint64_t* affine, int on_device, size_t n, mnt753_check_report* out, void* stream);
/* mnt753_check_points plus membership in the group of prime order r.  Arguments, n = 0 and the no-device behaviour as there.
 * group == MNT753_G1: the cofactor is 1 on both curves, the result is mnt753_check_points' own and no further kernel runs.
 * group == MNT753_G2: both twists have a large cofactor, a point on the twist need not be in G2.  One lane group (2 / 3 lanes) per
 * point; per point the first that applies: non-canonical; the identity (good); off the twist; psi(P) != [t - 1] P ->
 * MNT753_BAD_NOT_IN_SUBGROUP, with psi the twisted Frobenius and t - 1 = q - r the ate loop count -- an exact, deterministic test per
 * point (no random combination: DESIGN.md section 4.13), some 376 doubling and 190 addition steps on the twist.  Meant for the B2
 * entries of a parameter file and for beta_g2 / delta_g2 of a key. */
int mnt753_check_subgroup(int curve, int group, const uint64_t* affine, int on_device, size_t n, mnt753_check_report* out, void* stream);
/* n Fr elements of the curve: bad = the stored integer is >= r (MNT753_BAD_NONCANONICAL).  The field layer's contracts start from
 * canonical words (libff's Fp_model keeps them so, fp.tcc:161-186; a file can hold anything). */
int mnt753_check_scalars(int curve, const uint64_t* fr, int on_device, size_t n, mnt753_check_report* out, void* stream);
/* a[i] b[i] == c[i] in Fr for i < n on three device vectors: over the d + 1 entries of ca / cb / cc this is
 * r1cs_constraint_system::is_satisfied (r1cs.tcc: <a_i, w> <b_i, w> = <c_i, w> per constraint; the input-consistency rows hold
 * (w_i, 0, 0) and pass).  Right for any words: a row with an operand >= r is MNT753_BAD_NONCANONICAL, else a failing product is
 * MNT753_BAD_UNSATISFIED. */
int mnt753_check_products(int curve, const uint64_t* dev_a, const uint64_t* dev_b, const uint64_t* dev_c, size_t n, mnt753_check_report* out, void* stream);
/* cs.is_satisfied(primary_input, auxiliary_input) (r1cs_to_qap.tcc:216) for the assignment dev_w (m + 1 elements, w[0] = 1):
 * mnt753_r1cs_evaluate into scratch vectors, then mnt753_check_products; first_bad = the lowest unsatisfied constraint row. */
int mnt753_r1cs_check(mnt753_r1cs* r, const uint64_t* dev_w, mnt753_check_report* out, void* stream);

/* ---- compressed points (device; the stream records on the host) ------------------------------------------
 * libff's default point format (USE_PT_COMPRESSION; the challenge reference builds with NO_PT_COMPRESSION): x and one bit of y,
 * operator<< / operator>> of depends/libff/libff/algebra/curves/mnt753/mnt4753/mnt4753_g1.cpp:389-450, mnt4753_g2.cpp:419-460 and the
 * two mnt6753 files.  The PACKED compressed form of n points of (curve, group):
 *   x:     n x mnt753_compressed_words words, the x coordinate exactly as in the affine wire form (Montgomery words, c0 | c1 | c2);
 *   flags: n bytes; bit 0 = the parity of y as an INTEGER in [0, q), out of Montgomery form (G2: of y.c0) -- libff's
 *          Y.as_bigint().data[0] & 1; bit 1 = the identity; bits 2-7 zero.
 * mnt753_compress_points: affine wire points -> (x, flags); the identity (all words of y zero) gives x all zero and flag 2.  It
 * VALIDATES NOTHING, like libff's operator<<: a point off its curve is compressed as it stands.
 * mnt753_decompress_points: (x, flags) -> affine wire points and a report as mnt753_check_points fills it.  Per point, the first
 * rule that applies: a flag bit 2-7 set or a component of x >= q -> MNT753_BAD_NONCANONICAL; the identity flag -> zero words, good,
 * whatever x holds; x^3 + a x + b (G2: the twist's a', b') not a square, or zero -> MNT753_BAD_OFF_CURVE (for zero the only point has
 * y = 0, which the wire form reads as the identity and which lies in neither group); otherwise y is the root whose parity is bit 0.
 * A bad point's output is all-zero words, its neighbours are not disturbed.  The output goes straight into mnt753_bases_create.
 * One lane per G1 point, one lane group (2 / 3 lanes) per G2 point; the square root (csrc/fp_sqrt.hip.h) has
 * no data-dependent control flow.  A DEPARTURE from libff, in a case its format leaves open: for a G2 point with y.c0 = 0, y != 0 both
 * roots carry flag 0 and libff returns whichever its loop lands on; here it is the root whose first non-zero higher component is even,
 * whatever bit 0 says.
 * Conventions of the validation calls above: n = 0 gives an all-zero report, null pointers and bad ids are MNT753_EINVAL, no device
 * is MNT753_ENODEV, a malformed input is a result and not a failed call, on_device != 0: every pointer but the report is a device
 * pointer on the current device (16-byte aligned, as every wire array). */
size_t mnt753_compressed_words(int curve, int group);            /* 12, 24 (MNT4753 G2) or 36 (MNT6753 G2); 0 for bad ids */
int mnt753_compress_points(int curve, int group, const uint64_t* affine, int on_device, size_t n, uint64_t* x_out, uint8_t* flags_out, void* stream);
int mnt753_decompress_points(int curve, int group, const uint64_t* x, const uint8_t* flags, int on_device, size_t n, uint64_t* affine_out,
                             mnt753_check_report* out, void* stream);
/* mnt753_groth16_verify_ex on compressed proofs.  x: n x (x_A | x_B | x_C), 24 + mnt753_compressed_words(curve, MNT753_G2) words per
 * proof; flags: n x 3 bytes (A, B, C); inputs, on_device, verify_flags, verdicts, stream and the return value as there.  A chunk is
 * decompressed on the device into the affine staging buffer of the per-proof verifier, then the same kernels run: the verdicts are
 * those of mnt753_decompress_points followed by mnt753_groth16_verify_ex, where verdict 1 (malformed) also covers every decompression
 * failure and an identity flag on A, B or C.  Chunks stay under mnt753_vk_set_workspace_cap; per proof of a chunk, on top of the
 * 194 + 96 num_inputs bytes of mnt753_groth16_verify: 8 (48 + mnt753_affine_words(curve, MNT753_G2)) bytes for the decompressed proof
 * (768 / 960), and for a batch in host memory 8 (24 + compressed words of G2) + 3 (387 / 483) instead of the staged affine copy.
 * The folded verifier takes no compressed proofs. */
int mnt753_groth16_verify_compressed(const mnt753_vk* vk, const uint64_t* x /* n x (x_A|x_B|x_C) */, const uint8_t* flags /* n x 3 */,
                                     const uint64_t* inputs, size_t n, int on_device, unsigned verify_flags, uint8_t* verdicts, void* stream);
/* libff's stream records of the packed form, host only (no device needed): under BINARY_OUTPUT + MONTGOMERY_OUTPUT, where
 * OUTPUT_SEPARATOR is empty (serialization.hpp:63-66), one point is the byte '0' or '1' (is the identity), the 8 x compressed-words
 * bytes of x, and the byte '0' or '1' (the parity): 98, 194 (MNT4753 G2) or 290 (MNT6753 G2) bytes.  The identity is written as libff
 * writes its zero() after to_affine_coordinates(), X = 0 and Y = 1: '1', zero bytes, '1'; both parity bytes are accepted for it on
 * input, and it comes back as x all zero and flag 2.  A compressed proof is the three records A | B | C back to back (390 / 486
 * bytes; r1cs_gg_ppzksnark_proof::operator<< where OUTPUT_NEWLINE is empty).
 * to_stream: *len = the size; buf == NULL asks for the size alone; cap < *len, or a flag byte with a bit 2-7 set, is MNT753_EINVAL.
 * from_stream: any other byte in a flag position, or len < n records, is MNT753_EINVAL. */
int mnt753_points_to_stream(int curve, int group, const uint64_t* x, const uint8_t* flags, size_t n, uint8_t* buf, size_t cap, size_t* len);
int mnt753_points_from_stream(int curve, int group, const uint8_t* buf, size_t len, size_t n, uint64_t* x, uint8_t* flags);

/* ---- uniform scalars (host) ---------------------------------------------------------------------------
 * n elements of Fr of the curve, uniform in [0, r) by rejection on 753-bit draws of a seeded SplitMix64, in wire form.  What the
 * product needs them for: the scalars of the warm-up MSMs at parameter-load time (B::read_params) and the prover's second random
 * element s of `main_hip complete` when no file names one (main.cpp:312-319 draws it with libff's random_element). */
int mnt753_synth_scalars(int curve, uint64_t seed, size_t n, uint64_t* out_scalars);

/* The synthetic base points with known discrete logarithms and the device-level test hooks are NOT part of this library: they live
 * in libmnt753_hip_test.so (include/mnt753_hip_test.h), which tests/, bench.py and __graft_entry__.smoke() load beside it. */

#ifdef __cplusplus
}
#endif
#endif /* MNT753_HIP_H */
