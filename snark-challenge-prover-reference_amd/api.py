"""ctypes binding of include/mnt753_hip.h.  No compute happens in Python; every call lands in
libmnt753_hip.so, and the loader raises if the library was not built (no fallback path)."""
import ctypes as C
import os

import numpy as np

CURVE_MNT4753, CURVE_MNT6753 = 0, 1
G1, G2 = 1, 2
FFT, IFFT, COSET_FFT, ICOSET_FFT = 0, 1, 2, 3

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class Mnt753Error(RuntimeError):
    pass


BAD_NONE, BAD_NONCANONICAL, BAD_OFF_CURVE, BAD_UNSATISFIED = 0, 1, 2, 3
BAD_NOT_IN_SUBGROUP = 4
VERIFY_CHECK_SUBGROUP = 1


class QapPlan(C.Structure):
    """mnt753_qap_plan"""
    _fields_ = [("chunk_terms", C.c_uint32), ("reserved", C.c_uint32), ("terms", C.c_uint64), ("work_items", C.c_uint64),
                ("split_columns", C.c_uint64), ("longest_column", C.c_uint64), ("transpose_bytes", C.c_uint64), ("partial_bytes", C.c_uint64)]


class CheckReport(C.Structure):
    """mnt753_check_report"""
    _fields_ = [("n_bad", C.c_uint64), ("first_bad", C.c_uint64), ("first_reason", C.c_uint32), ("reserved", C.c_uint32)]


class VkInputPlan(C.Structure):
    """mnt753_vk_input_plan_t"""
    _fields_ = [("window_bits", C.c_int), ("windows", C.c_int), ("inputs_per_lane", C.c_uint32), ("reserved", C.c_uint32),
                ("table_bytes", C.c_uint64), ("prepared", C.c_int), ("reserved2", C.c_int)]


class KeygenSizes(C.Structure):
    """mnt753_keygen_sizes"""
    _fields_ = [(k, C.c_uint64) for k in ("a_query", "b_g1_query", "b_g2_query", "l_query", "h_query", "abc_g1")]


class KeygenOut(C.Structure):
    """mnt753_keygen_out"""
    _fields_ = [(k, C.c_void_p) for k in ("dev_a_query", "dev_b_g1_query", "dev_b_g2_query", "dev_l_query", "dev_h_query", "dev_abc_g1",
                                          "host_alpha_g1", "host_beta_g1", "host_beta_g2", "host_delta_g1", "host_delta_g2")]


class KeygenOpts(C.Structure):
    """mnt753_keygen_opts"""
    _fields_ = [("g1_window_bits", C.c_int), ("g2_window_bits", C.c_int), ("g1_tile", C.c_size_t), ("g2_tile", C.c_size_t),
                ("flags", C.c_uint), ("reserved", C.c_uint)]


class KeygenReport(C.Structure):
    """mnt753_keygen_report"""
    _fields_ = [("non_zero_at", C.c_uint64), ("non_zero_bt", C.c_uint64), ("swapped", C.c_int), ("reserved", C.c_int)]


KEYGEN_DENSE_G1, KEYGEN_DENSE_G2 = 1, 2


class HCheckResult(C.Structure):
    """mnt753_h_check_result: the verdict of H(t) Z(t) = A(t) B(t) - C(t) and its two sides in wire form"""
    _fields_ = [("ok", C.c_int32), ("reserved", C.c_int32), ("lhs", C.c_uint64 * 12), ("rhs", C.c_uint64 * 12)]


class FoldLocateReport(C.Structure):
    """mnt753_fold_locate_report"""
    _fields_ = [("segments", C.c_uint64), ("segments_rejected", C.c_uint64), ("proofs_rechecked", C.c_uint64), ("ms_scale", C.c_float),
                ("ms_miller", C.c_float), ("ms_tails", C.c_float), ("ms_recheck", C.c_float)]

    def as_dict(self):
        return {"segments": int(self.segments), "segments_rejected": int(self.segments_rejected), "proofs_rechecked": int(self.proofs_rechecked),
                "ms_scale": float(self.ms_scale), "ms_miller": float(self.ms_miller), "ms_tails": float(self.ms_tails),
                "ms_recheck": float(self.ms_recheck)}


# Names an OLDER build of the library may lack: empty in the product.  An A/B tool that times a build from before a call existed
# (tools/bench_fold.py with MNT753_LIB) adds the name here before the first lib(); every other name must resolve.
OPTIONAL_SYMBOLS = set()


def lib_path():
    """The product library next to this file; MNT753_LIB names another build of it (development A/B runs: an experimental
    variant is loaded from where it was built instead of being copied over the product file)."""
    return os.environ.get("MNT753_LIB") or os.path.join(_HERE, "libmnt753_hip.so")


def lib():
    """Load libmnt753_hip.so (built by `make` / __graft_entry__.build()); fail loudly if missing."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise Mnt753Error(f"{path} not found: build the HIP extension first (make, or __graft_entry__.build())")
    # RTLD_GLOBAL: the test library beside it (test_lib) names the product by its soname and must find THIS copy -- also when
    # MNT753_LIB loaded a development variant from another directory
    L = C.CDLL(path, mode=C.RTLD_GLOBAL)
    u64p, vp, sz, i = C.POINTER(C.c_uint64), C.c_void_p, C.c_size_t, C.c_int
    sig = {
        "mnt753_init": (i, [i]),
        "mnt753_init_devices": (i, [i]),
        "mnt753_device_count": (i, []),
        "mnt753_set_device": (i, [i]),
        "mnt753_get_device": (i, []),
        "mnt753_enable_peer_access": (i, [i, i, C.POINTER(C.c_int)]),
        "mnt753_copy_peer": (i, [i, vp, i, vp, sz]),
        "mnt753_copy_peer_async": (i, [i, vp, i, vp, sz]),
        "mnt753_last_error": (C.c_char_p, []),
        "mnt753_exchange_points": (i, [C.POINTER(vp), sz, u64p]),
        "mnt753_exchange_last_us": (C.c_double, []),
        "mnt753_affine_words": (sz, [i, i]),
        "mnt753_projective_words": (sz, [i, i]),
        "mnt753_dev_alloc": (i, [C.POINTER(vp), sz]),
        "mnt753_dev_free": (i, [vp]),
        "mnt753_copy_h2d": (i, [vp, vp, sz]),
        "mnt753_copy_d2h": (i, [vp, vp, sz]),
        "mnt753_copy_d2d": (i, [vp, vp, sz]),
        "mnt753_dev_memset": (i, [vp, i, sz]),
        "mnt753_sync": (i, [vp]),
        "mnt753_load_file_to_device": (i, [C.c_char_p, sz, sz, vp]),
        "mnt753_bases_create": (i, [i, i, vp, i, sz, C.POINTER(vp)]),
        "mnt753_bases_free": (i, [vp]),
        "mnt753_bases_size": (sz, [vp]),
        "mnt753_msm": (i, [vp, sz, vp, i, sz, u64p, vp]),
        "mnt753_msm_start": (i, [vp, sz, vp, i, sz, vp]),
        "mnt753_msm_finish": (i, [vp, u64p]),
        "mnt753_msm_set_window_bits": (i, [i]),
        "mnt753_msm_set_window_table": (i, [i]),
        "mnt753_dev_mem_info": (i, [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
        "mnt753_self_test": (i, [i]),
        "mnt753_self_test_curve": (i, [i, i]),
        "mnt753_msm_order_after": (i, [vp, vp]),
        "mnt753_msm_last_timing": (i, [C.POINTER(C.c_float)]),
        "mnt753_msm_last_plan": (i, [C.POINTER(C.c_int)]),
        "mnt753_msm_last_pair_levels": (i, []),
        "mnt753_msm_last_irr_levels": (i, []),
        "mnt753_point_add": (i, [i, i, u64p, u64p, u64p]),
        "mnt753_point_scale": (i, [i, i, u64p, u64p, u64p]),
        "mnt753_point_to_affine": (i, [i, i, u64p, u64p]),
        "mnt753_point_from_affine": (i, [i, i, u64p, u64p]),
        "mnt753_domain_create": (i, [i, sz, C.POINTER(vp)]),
        "mnt753_domain_create_for": (i, [i, sz, C.POINTER(vp)]),
        "mnt753_domain_create_for_ex": (i, [i, sz, C.c_uint, C.POINTER(vp)]),
        "mnt753_domain_create_mixed": (i, [i, sz, C.POINTER(vp)]),
        "mnt753_domain_kind": (i, [vp]),
        "mnt753_domain_free": (i, [vp]),
        "mnt753_domain_size": (sz, [vp]),
        "mnt753_fft": (i, [vp, i, vp, vp]),
        "mnt753_divide_by_z_on_coset": (i, [vp, vp, vp]),
        "mnt753_vec_muleq": (i, [i, vp, vp, sz, vp]),
        "mnt753_vec_subeq": (i, [i, vp, vp, sz, vp]),
        "mnt753_vec_scale": (i, [i, vp, vp, vp, sz, vp]),
        "mnt753_compute_h": (i, [vp, vp, vp, vp, vp, vp]),
        "mnt753_compute_h_chain": (i, [vp, vp, vp]),
        "mnt753_compute_h_finish": (i, [vp, vp, vp, vp, vp, vp]),
        "mnt753_domain_device": (i, [vp]),
        "mnt753_domain_vanishing_at": (i, [vp, u64p, u64p]),
        "mnt753_domain_lagrange_at": (i, [vp, u64p, vp, vp]),
        "mnt753_vec_powers": (i, [i, u64p, vp, sz, vp]),
        "mnt753_vec_dot": (i, [i, vp, vp, sz, u64p, vp]),
        "mnt753_poly_eval": (i, [i, vp, sz, u64p, u64p, vp]),
        "mnt753_domain_interp_at": (i, [vp, u64p, C.POINTER(vp), i, vp, u64p, vp]),
        "mnt753_h_check": (i, [vp, u64p, u64p, vp, C.POINTER(HCheckResult), vp]),
        "mnt753_compute_h_checked": (i, [vp, vp, vp, vp, vp, u64p, C.POINTER(HCheckResult), vp]),
        "mnt753_r1cs_qap_plan": (i, [vp, C.POINTER(QapPlan)]),
        "mnt753_r1cs_qap_at": (i, [vp, vp, u64p, vp, vp, vp, vp, u64p, vp]),
        "mnt753_synth_scalars": (i, [i, C.c_uint64, sz, u64p]),
        "mnt753_r1cs_create": (i, [i, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]),
        "mnt753_r1cs_free": (i, [vp]),
        "mnt753_r1cs_domain_size": (sz, [vp]),
        "mnt753_r1cs_num_variables": (sz, [vp]),
        "mnt753_r1cs_num_inputs": (sz, [vp]),
        "mnt753_r1cs_evaluate": (i, [vp, vp, vp, vp, vp, sz, vp]),
        "mnt753_check_points": (i, [i, i, vp, i, sz, C.POINTER(CheckReport), vp]),
        "mnt753_check_subgroup": (i, [i, i, vp, i, sz, C.POINTER(CheckReport), vp]),
        "mnt753_check_scalars": (i, [i, vp, i, sz, C.POINTER(CheckReport), vp]),
        "mnt753_check_products": (i, [i, vp, vp, vp, sz, C.POINTER(CheckReport), vp]),
        "mnt753_r1cs_check": (i, [vp, vp, C.POINTER(CheckReport), vp]),
        "mnt753_fixed_base_create": (i, [i, i, vp, i, sz, C.POINTER(vp)]),
        "mnt753_fixed_base_free": (i, [vp]),
        "mnt753_fixed_base_plan": (i, [vp, C.POINTER(C.c_int)]),
        "mnt753_fixed_base_table_bytes": (sz, [vp]),
        "mnt753_fixed_base_last_timing": (i, [vp, C.POINTER(C.c_float)]),
        "mnt753_batch_exp": (i, [vp, vp, i, sz, vp, vp, i, vp]),
        "mnt753_r1cs_swap_ab_if_beneficial": (i, [vp, C.POINTER(C.c_int)]),
        "mnt753_r1cs_is_swapped": (i, [vp]),
        "mnt753_compact_nonzero": (i, [vp, sz, vp, vp, C.POINTER(C.c_size_t), vp]),
        "mnt753_scatter_rows": (i, [vp, vp, sz, sz, vp, sz, vp]),
        "mnt753_batch_exp_sparse": (i, [vp, vp, sz, vp, vp, C.POINTER(C.c_size_t), vp]),
        "mnt753_keygen_combine": (i, [i, vp, vp, vp, sz, sz, u64p, u64p, u64p, vp, vp]),
        "mnt753_groth16_sizes": (i, [vp, vp, C.POINTER(KeygenSizes)]),
        "mnt753_groth16_generate": (i, [vp, vp, u64p, u64p, u64p, u64p, u64p, C.POINTER(KeygenOpts), C.POINTER(KeygenOut), C.POINTER(KeygenReport), vp]),
        "mnt753_group_generator": (i, [i, i, u64p]),
        "mnt753_gt_words": (sz, [i]),
        "mnt753_pairing": (i, [i, vp, vp, sz, i, vp, vp]),
        "mnt753_vk_create": (i, [i, u64p, u64p, u64p, u64p, sz, C.POINTER(vp)]),
        "mnt753_vk_destroy": (i, [vp]),
        "mnt753_vk_num_inputs": (sz, [vp]),
        "mnt753_vk_coefficient_bytes": (sz, [vp]),
        "mnt753_vk_set_workspace_cap": (i, [vp, sz]),
        "mnt753_vk_gt": (i, [vp, u64p]),
        "mnt753_vk_serialize": (i, [vp, vp, sz, C.POINTER(C.c_size_t)]),
        "mnt753_vk_accumulate": (i, [vp, u64p, sz, u64p]),
        "mnt753_vk_prepare_inputs": (i, [vp, i, sz]),
        "mnt753_vk_input_plan": (i, [vp, sz, C.POINTER(VkInputPlan)]),
        "mnt753_vk_release_inputs": (i, [vp]),
        "mnt753_groth16_verify": (i, [vp, vp, vp, sz, i, vp, vp]),
        "mnt753_groth16_verify_ex": (i, [vp, vp, vp, sz, i, C.c_uint, vp, vp]),
        "mnt753_groth16_verify_folded": (i, [vp, vp, vp, sz, i, u64p, vp, C.POINTER(C.c_int), vp]),
        "mnt753_fold_segment_proofs": (sz, [i]),
        "mnt753_groth16_verify_folded_locate": (i, [vp, vp, vp, sz, i, u64p, vp, C.POINTER(FoldLocateReport), vp]),
        "mnt753_compressed_words": (sz, [i, i]),
        "mnt753_compress_points": (i, [i, i, vp, i, sz, vp, vp, vp]),
        "mnt753_decompress_points": (i, [i, i, vp, vp, i, sz, vp, C.POINTER(CheckReport), vp]),
        "mnt753_groth16_verify_compressed": (i, [vp, vp, vp, vp, sz, i, C.c_uint, vp, vp]),
        "mnt753_points_to_stream": (i, [i, i, vp, vp, sz, vp, sz, C.POINTER(C.c_size_t)]),
        "mnt753_points_from_stream": (i, [i, i, vp, sz, sz, vp, vp]),
    }
    for name, (res, args) in sig.items():
        if name in OPTIONAL_SYMBOLS and not hasattr(L, name):
            continue
        fn = getattr(L, name)   # AttributeError here = the library does not export what the header declares
        fn.restype, fn.argtypes = res, args
    _LIB = L
    return L


_TEST_LIB = None


def test_lib_path():
    return os.environ.get("MNT753_TEST_LIB") or os.path.join(_HERE, "libmnt753_hip_test.so")


def test_lib():
    """libmnt753_hip_test.so (include/mnt753_hip_test.h): synthetic bases with known discrete logarithms and the device-level
    known-answer hooks.  Test infrastructure: tests/, bench.py and __graft_entry__.smoke() load it, the product never does."""
    global _TEST_LIB
    if _TEST_LIB is not None:
        return _TEST_LIB
    lib()   # the product first: the test library resolves set_error / require_device and the HIP state against it
    path = test_lib_path()
    if not os.path.exists(path):
        raise Mnt753Error(f"{path} not found: build the HIP extension first (make, or __graft_entry__.build())")
    L = C.CDLL(path)
    u64p, u32p, sz, i = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.c_size_t, C.c_int
    sig = {
        "mnt753_synth_points": (i, [i, i, C.c_uint64, sz, u64p, i]),
        "mnt753_synth_expected_msm": (i, [i, i, C.c_uint64, sz, u64p, u64p]),
        "mnt753_test_generator": (i, [i, i, u64p]),
        "mnt753_test_field_op": (i, [i, i, u64p, u64p, sz, u64p]),
        "mnt753_test_ext_op": (i, [i, i, i, u64p, u64p, sz, u64p]),
        "mnt753_test_point_op": (i, [i, i, i, i, u64p, u64p, sz, u64p]),
        "mnt753_test_field_raw": (i, [i, i, u32p, sz, C.c_uint32, u32p]),
        "mnt753_test_ext_raw": (i, [i, i, i, u32p, u32p, sz, u32p]),
        "mnt753_test_tower_op": (i, [i, i, i, u64p, u64p, sz, u64p]),
        "mnt753_test_miller_loop": (i, [i, i, u64p, u64p, sz, u64p]),
        "mnt753_test_g2_endomorphism": (i, [i, u64p, sz, u64p]),
        "mnt753_test_g2_loop_multiple": (i, [i, u64p, sz, u64p]),
        "mnt753_test_reduce_capped": (i, [i, i, C.c_void_p, C.c_void_p, sz, u64p, C.c_uint, u64p]),
        "mnt753_test_fold_parts": (i, [C.c_void_p, u64p, u64p, sz, u64p, u64p, u64p, u64p, u64p, C.c_void_p, C.POINTER(C.c_int)]),
        "mnt753_test_fold_segment_parts": (i, [C.c_void_p, u64p, u64p, sz, u64p, u64p, u64p, u64p, u64p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.POINTER(FoldLocateReport)]),
        "mnt753_test_fold_locate_last_chunks": (C.c_size_t, []),
        "mnt753_test_fold_last_timing": (i, [C.POINTER(C.c_float)]),
        "mnt753_test_vk_force_inputs_per_lane": (i, [C.c_void_p, C.c_uint32]),
        "mnt753_test_vk_inputs_last_timing": (i, [C.c_void_p, C.POINTER(C.c_float)]),
        "mnt753_test_vk_set_gt": (i, [C.c_void_p, u64p]),
        "mnt753_test_field_sqrt": (i, [i, i, u64p, sz, u64p, C.c_void_p]),
        "mnt753_test_field_sqrt_window": (i, [i, i, i, u64p, sz, u64p, C.c_void_p, C.POINTER(C.c_float)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    _TEST_LIB = L
    return L


def _check(rc, what):
    if rc != 0:
        raise Mnt753Error(f"{what} failed (rc={rc}): {lib().mnt753_last_error().decode()}")


def _u64(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return a, a.ctypes.data_as(C.POINTER(C.c_uint64))


def init(device=0):
    _check(lib().mnt753_init(int(device)), "mnt753_init")


def self_test(level=1, curve=None):
    """mnt753_self_test / _curve: the known answers embedded in the library (include/mnt753_hip.h); raises Mnt753Error on a mismatch"""
    if curve is None:
        _check(lib().mnt753_self_test(level), "mnt753_self_test")
    else:
        _check(lib().mnt753_self_test_curve(curve, level), "mnt753_self_test")


def exchange_points(blocks):
    """all-gather of one block of u64 words per logical device over RCCL inside the boundary (mnt753_exchange_points);
    returns (list of blocks in rank order, microseconds)."""
    keep = [np.ascontiguousarray(b, dtype=np.uint64) for b in blocks]
    words = keep[0].size
    arr = (C.c_void_p * len(keep))(*[C.c_void_p(k.ctypes.data) for k in keep])
    out = np.zeros(len(keep) * words, dtype=np.uint64)
    _check(lib().mnt753_exchange_points(arr, words, out.ctypes.data_as(C.POINTER(C.c_uint64))), "mnt753_exchange_points")
    return [out[g * words:(g + 1) * words].copy() for g in range(len(keep))], float(lib().mnt753_exchange_last_us())


def affine_words(curve, group):
    return int(lib().mnt753_affine_words(curve, group))


def projective_words(curve, group):
    return int(lib().mnt753_projective_words(curve, group))


class BaseSet:
    """Device-resident vector_G1 / vector_G2 (B::params_A ... of the reference)."""

    def __init__(self, curve, group, affine, on_device=False, n=None):
        self.curve, self.group = curve, group
        self._h = C.c_void_p()
        if on_device:
            ptr, cnt = C.c_void_p(int(affine)), int(n)
        else:
            self._keep = np.ascontiguousarray(affine, dtype=np.uint64)
            cnt = self._keep.size // affine_words(curve, group) if n is None else int(n)
            ptr = C.c_void_p(self._keep.ctypes.data)
        _check(lib().mnt753_bases_create(curve, group, ptr, 1 if on_device else 0, cnt, C.byref(self._h)), "mnt753_bases_create")
        self.n = cnt

    def msm(self, scalars, n=None, base_offset=0, on_device=False, stream=None):
        """sum scalars[i] * bases[base_offset + i]; returns the projective wire words (numpy u64)."""
        out = np.zeros(projective_words(self.curve, self.group), dtype=np.uint64)
        if on_device:
            sptr, cnt = C.c_void_p(int(scalars)), int(n)
        else:
            keep = np.ascontiguousarray(scalars, dtype=np.uint64)
            cnt = keep.size // 12 if n is None else int(n)
            sptr = C.c_void_p(keep.ctypes.data)
        st = C.c_void_p(int(stream)) if stream else C.c_void_p()
        _check(lib().mnt753_msm(self._h, base_offset, sptr, 1 if on_device else 0, cnt,
                                out.ctypes.data_as(C.POINTER(C.c_uint64)), st), "mnt753_msm")
        return out

    def msm_start(self, scalars_dev_ptr, n, base_offset=0, stream=None):
        """Enqueue sum scalars[i] * bases[base_offset + i] (scalars resident on the device); collect with msm_finish()."""
        st = C.c_void_p(int(stream)) if stream else C.c_void_p()
        _check(lib().mnt753_msm_start(self._h, base_offset, C.c_void_p(int(scalars_dev_ptr)), 1, int(n), st), "mnt753_msm_start")

    def order_after(self, first):
        """The point kernels of this set's NEXT msm_start begin when those of `first`'s MSM in flight have ended (mnt753_msm_order_after)."""
        _check(lib().mnt753_msm_order_after(self._h, first._h), "mnt753_msm_order_after")

    def msm_finish(self):
        out = np.zeros(projective_words(self.curve, self.group), dtype=np.uint64)
        _check(lib().mnt753_msm_finish(self._h, out.ctypes.data_as(C.POINTER(C.c_uint64))), "mnt753_msm_finish")
        return out

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().mnt753_bases_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def msm_last_timing():
    t = (C.c_float * 5)()
    _check(lib().mnt753_msm_last_timing(t), "mnt753_msm_last_timing")
    return dict(total_ms=t[0], sort_ms=t[1], accumulate_ms=t[2], reduce_ms=t[3], host_ms=t[4])


def msm_last_plan():
    t = (C.c_int * 4)()
    _check(lib().mnt753_msm_last_plan(t), "mnt753_msm_last_plan")
    return dict(window_bits=t[0], windows=t[1], window_table=bool(t[2]), entries_per_lane=t[3],
                pair_levels=int(lib().mnt753_msm_last_pair_levels()), irr_levels=int(lib().mnt753_msm_last_irr_levels()))


def point_add(curve, group, a, b):
    a, pa = _u64(a); b, pb = _u64(b)
    out = np.zeros(projective_words(curve, group), dtype=np.uint64)
    _check(lib().mnt753_point_add(curve, group, pa, pb, out.ctypes.data_as(C.POINTER(C.c_uint64))), "mnt753_point_add")
    return out


def point_scale(curve, group, scalar, p):
    s, ps = _u64(scalar); p, pp = _u64(p)
    out = np.zeros(projective_words(curve, group), dtype=np.uint64)
    _check(lib().mnt753_point_scale(curve, group, ps, pp, out.ctypes.data_as(C.POINTER(C.c_uint64))), "mnt753_point_scale")
    return out


def point_to_affine(curve, group, p):
    p, pp = _u64(p)
    out = np.zeros(affine_words(curve, group), dtype=np.uint64)
    _check(lib().mnt753_point_to_affine(curve, group, pp, out.ctypes.data_as(C.POINTER(C.c_uint64))), "mnt753_point_to_affine")
    return out


def point_from_affine(curve, group, a):
    a, pa = _u64(a)
    out = np.zeros(projective_words(curve, group), dtype=np.uint64)
    _check(lib().mnt753_point_from_affine(curve, group, pa, out.ctypes.data_as(C.POINTER(C.c_uint64))), "mnt753_point_from_affine")
    return out


class DeviceBuffer:
    """Device memory owned through the C ABI (for callers without torch)."""

    def __init__(self, nbytes):
        self.ptr = C.c_void_p()
        self.nbytes = int(nbytes)
        _check(lib().mnt753_dev_alloc(C.byref(self.ptr), self.nbytes), "mnt753_dev_alloc")

    @classmethod
    def from_numpy(cls, a):
        a = np.ascontiguousarray(a)
        b = cls(a.nbytes)
        _check(lib().mnt753_copy_h2d(b.ptr, C.c_void_p(a.ctypes.data), a.nbytes), "mnt753_copy_h2d")
        return b

    @classmethod
    def from_file(cls, path, offset, nbytes):
        """Stream nbytes of a file (from byte offset) into new device memory (mnt753_load_file_to_device)."""
        b = cls(nbytes)
        _check(lib().mnt753_load_file_to_device(str(path).encode(), int(offset), int(nbytes), b.ptr), "mnt753_load_file_to_device")
        return b

    def to_numpy(self, dtype=np.uint64):
        out = np.zeros(self.nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        _check(lib().mnt753_copy_d2h(C.c_void_p(out.ctypes.data), self.ptr, self.nbytes), "mnt753_copy_d2h")
        return out

    def close(self):
        if self.ptr and self.ptr.value:
            lib().mnt753_dev_free(self.ptr)
            self.ptr = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Domain:
    """An evaluation domain over Fr of the curve.  Domain(curve, m): libfqfft's basic_radix2_domain of exactly m elements (a power of
    two).  Domain.for_size(curve, min_size): the domain libfqfft's get_evaluation_domain(min_size) builds (B::get_evaluation_domain) --
    basic, extended (2^(s+1)) or step (2^k + 2^r) radix-2; its size `m` may be larger than min_size.  With mixed=True the walk also
    builds the mixed-radix basic domains of MNT6753 (2^a 5^b, a <= 15, b <= 2: up to 819200 elements) where it otherwise stops with
    an error.  Domain.mixed(curve, m): that domain at exactly m elements."""

    BASIC, EXTENDED, STEP, MIXED = 0, 1, 2, 3
    ALLOW_MIXED = 1

    def __init__(self, curve, m):
        self.curve, self.m = curve, int(m)
        self._h = C.c_void_p()
        _check(lib().mnt753_domain_create(curve, self.m, C.byref(self._h)), "mnt753_domain_create")

    @classmethod
    def for_size(cls, curve, min_size, mixed=False):
        self = cls.__new__(cls)
        self.curve = curve
        self._h = C.c_void_p()
        if mixed:
            _check(lib().mnt753_domain_create_for_ex(curve, int(min_size), cls.ALLOW_MIXED, C.byref(self._h)), "mnt753_domain_create_for_ex")
        else:
            _check(lib().mnt753_domain_create_for(curve, int(min_size), C.byref(self._h)), "mnt753_domain_create_for")
        self.m = int(lib().mnt753_domain_size(self._h))
        return self

    @classmethod
    def mixed(cls, curve, m):
        self = cls.__new__(cls)
        self.curve, self.m = curve, int(m)
        self._h = C.c_void_p()
        _check(lib().mnt753_domain_create_mixed(curve, self.m, C.byref(self._h)), "mnt753_domain_create_mixed")
        return self

    @property
    def kind(self):
        """Domain.BASIC, Domain.EXTENDED, Domain.STEP or Domain.MIXED."""
        return int(lib().mnt753_domain_kind(self._h))

    def fft(self, kind, dev_ptr, stream=None):
        st = C.c_void_p(int(stream)) if stream else C.c_void_p()
        _check(lib().mnt753_fft(self._h, kind, C.c_void_p(int(dev_ptr)), st), "mnt753_fft")

    def divide_by_z_on_coset(self, dev_ptr, stream=None):
        st = C.c_void_p(int(stream)) if stream else C.c_void_p()
        _check(lib().mnt753_divide_by_z_on_coset(self._h, C.c_void_p(int(dev_ptr)), st), "mnt753_divide_by_z_on_coset")

    def compute_h(self, ca, cb, cc, h, stream=None):
        st = C.c_void_p(int(stream)) if stream else C.c_void_p()
        _check(lib().mnt753_compute_h(self._h, C.c_void_p(int(ca)), C.c_void_p(int(cb)), C.c_void_p(int(cc)),
                                      C.c_void_p(int(h)), st), "mnt753_compute_h")

    def compute_h_chain(self, vec, stream=None):
        """vec <- cosetFFT(iFFT(vec)): the per-vector half of compute_H (runs on the domain's device)."""
        st = C.c_void_p(int(stream)) if stream else C.c_void_p()
        _check(lib().mnt753_compute_h_chain(self._h, C.c_void_p(int(vec)), st), "mnt753_compute_h_chain")

    def compute_h_finish(self, a, b, c, h, stream=None):
        """a <- icosetFFT((a * b - c) / Z), h <- a | 0: the joining half of compute_H."""
        st = C.c_void_p(int(stream)) if stream else C.c_void_p()
        _check(lib().mnt753_compute_h_finish(self._h, C.c_void_p(int(a)), C.c_void_p(int(b)), C.c_void_p(int(c)), C.c_void_p(int(h)), st),
               "mnt753_compute_h_finish")

    def vanishing_at(self, t):
        """Z(t) of the domain (compute_vanishing_polynomial): t and the result are 12 uint64 in wire form, on the host."""
        k, pk = _fr_elem(t)
        out = np.zeros(12, dtype=np.uint64)
        _check(lib().mnt753_domain_vanishing_at(self._h, pk, out.ctypes.data_as(C.POINTER(C.c_uint64))), "mnt753_domain_vanishing_at")
        return out

    def lagrange_at(self, t, out_ptr=None, stream=None):
        """The m Lagrange coefficients L_i(t) of the domain (evaluate_all_lagrange_polynomials).  Without out_ptr they come back as a
        numpy array [m, 12]; with out_ptr (a device address with room for m elements) they stay on the device and the call returns None."""
        k, pk = _fr_elem(t)
        st = C.c_void_p(int(stream)) if stream else C.c_void_p()
        if out_ptr is not None:
            _check(lib().mnt753_domain_lagrange_at(self._h, pk, C.c_void_p(int(out_ptr)), st), "mnt753_domain_lagrange_at")
            return None
        buf = DeviceBuffer(96 * self.m)
        try:
            _check(lib().mnt753_domain_lagrange_at(self._h, pk, buf.ptr, st), "mnt753_domain_lagrange_at")
            _check(lib().mnt753_sync(st), "mnt753_sync")
            return buf.to_numpy().reshape(self.m, 12)
        finally:
            buf.close()

    def interp_at(self, t, vecs, u_ptr=None, stream=None):
        """The values at t of the polynomials (1 to 3 of them, degree < m) that take vecs[j][i] at the domain's i-th element
        (mnt753_domain_interp_at): vecs are device addresses of m elements each, the result a numpy array [len(vecs), 12].  u_ptr: m
        elements of device scratch that receive L(t); without it the call brings its own."""
        k, pk = _fr_elem(t)
        st = C.c_void_p(int(stream)) if stream else C.c_void_p()
        arr = (C.c_void_p * len(vecs))(*[int(v) for v in vecs])
        out = np.zeros((len(vecs), 12), dtype=np.uint64)
        buf = DeviceBuffer(96 * self.m) if u_ptr is None else None
        try:
            u = buf.ptr if buf is not None else C.c_void_p(int(u_ptr))
            _check(lib().mnt753_domain_interp_at(self._h, pk, arr, len(vecs), u, out.ctypes.data_as(C.POINTER(C.c_uint64)), st),
                   "mnt753_domain_interp_at")
        finally:
            if buf is not None:
                buf.close()
        return out

    def h_check(self, t, abc, h, stream=None):
        """After compute_h: (ok, lhs, rhs) of H(t) Z(t) = A(t) B(t) - C(t) (mnt753_h_check).  abc: A(t) | B(t) | C(t) as interp_at
        returned them BEFORE compute_h overwrote the vectors; h: the device address of the m + 1 coefficients."""
        k, pk = _fr_elem(t)
        st = C.c_void_p(int(stream)) if stream else C.c_void_p()
        a = np.ascontiguousarray(abc, dtype=np.uint64).reshape(-1)
        assert a.size == 36
        res = HCheckResult()
        _check(lib().mnt753_h_check(self._h, pk, a.ctypes.data_as(C.POINTER(C.c_uint64)), C.c_void_p(int(h)), C.byref(res), st), "mnt753_h_check")
        return bool(res.ok), np.array(res.lhs, dtype=np.uint64), np.array(res.rhs, dtype=np.uint64)

    def compute_h_checked(self, ca, cb, cc, h, t=None, stream=None):
        """compute_h with the spot check around it (mnt753_compute_h_checked): (ok, lhs, rhs).  t=None: a random point from the
        operating system."""
        st = C.c_void_p(int(stream)) if stream else C.c_void_p()
        pk = None
        if t is not None:
            k, pk = _fr_elem(t)
        res = HCheckResult()
        _check(lib().mnt753_compute_h_checked(self._h, C.c_void_p(int(ca)), C.c_void_p(int(cb)), C.c_void_p(int(cc)), C.c_void_p(int(h)),
                                              pk, C.byref(res), st), "mnt753_compute_h_checked")
        return bool(res.ok), np.array(res.lhs, dtype=np.uint64), np.array(res.rhs, dtype=np.uint64)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().mnt753_domain_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _fr_elem(t):
    """one Fr element in wire form -> (array to keep alive, uint64 pointer)"""
    k = np.ascontiguousarray(t, dtype=np.uint64).reshape(-1)
    assert k.size == 12
    return k, k.ctypes.data_as(C.POINTER(C.c_uint64))


def vec_powers(curve, t, n, out_ptr=None, stream=None):
    """1, t, .., t^(n-1) in Fr of the curve (mnt753_vec_powers); a numpy array [n, 12], or None with out_ptr (a device address)."""
    k, pk = _fr_elem(t)
    st = C.c_void_p(int(stream)) if stream else C.c_void_p()
    if out_ptr is not None:
        _check(lib().mnt753_vec_powers(curve, pk, C.c_void_p(int(out_ptr)), int(n), st), "mnt753_vec_powers")
        return None
    buf = DeviceBuffer(96 * max(int(n), 1))
    try:
        _check(lib().mnt753_vec_powers(curve, pk, buf.ptr, int(n), st), "mnt753_vec_powers")
        _check(lib().mnt753_sync(st), "mnt753_sync")
        return buf.to_numpy().reshape(-1, 12)[:int(n)]
    finally:
        buf.close()


def vec_dot(curve, a_ptr, b_ptr, n, stream=None):
    """sum a[i] b[i] over n elements of Fr on the device (mnt753_vec_dot): 12 uint64 in wire form; a_ptr may equal b_ptr."""
    st = C.c_void_p(int(stream)) if stream else C.c_void_p()
    out = np.zeros(12, dtype=np.uint64)
    _check(lib().mnt753_vec_dot(curve, C.c_void_p(int(a_ptr)), C.c_void_p(int(b_ptr)), int(n), out.ctypes.data_as(C.POINTER(C.c_uint64)), st),
           "mnt753_vec_dot")
    return out


def poly_eval(curve, coeffs_ptr, n, t, stream=None):
    """sum c[i] t^i over n coefficients on the device (mnt753_poly_eval): 12 uint64 in wire form."""
    k, pk = _fr_elem(t)
    st = C.c_void_p(int(stream)) if stream else C.c_void_p()
    out = np.zeros(12, dtype=np.uint64)
    _check(lib().mnt753_poly_eval(curve, C.c_void_p(int(coeffs_ptr)), int(n), pk, out.ctypes.data_as(C.POINTER(C.c_uint64)), st), "mnt753_poly_eval")
    return out


def vec_muleq(curve, a_ptr, b_ptr, n, stream=None):
    st = C.c_void_p(int(stream)) if stream else C.c_void_p()
    _check(lib().mnt753_vec_muleq(curve, C.c_void_p(int(a_ptr)), C.c_void_p(int(b_ptr)), n, st), "mnt753_vec_muleq")


def copy_d2d(dst_ptr, src_ptr, nbytes):
    """Asynchronous device-to-device copy on the default stream (mnt753_copy_d2d)."""
    _check(lib().mnt753_copy_d2d(C.c_void_p(int(dst_ptr)), C.c_void_p(int(src_ptr)), int(nbytes)), "mnt753_copy_d2d")


def vec_scale(curve, dst_ptr, src_ptr, scalar, n, stream=None):
    """dst[i] = src[i] * scalar (scalar: 12 uint64 on the host, wire format)."""
    st = C.c_void_p(int(stream)) if stream else C.c_void_p()
    k = np.ascontiguousarray(scalar, dtype=np.uint64)
    assert k.size == 12
    _check(lib().mnt753_vec_scale(curve, C.c_void_p(int(dst_ptr)), C.c_void_p(int(src_ptr)), k.ctypes.data_as(C.c_void_p), n, st), "mnt753_vec_scale")


def vec_subeq(curve, a_ptr, b_ptr, n, stream=None):
    st = C.c_void_p(int(stream)) if stream else C.c_void_p()
    _check(lib().mnt753_vec_subeq(curve, C.c_void_p(int(a_ptr)), C.c_void_p(int(b_ptr)), n, st), "mnt753_vec_subeq")


def synth_points(curve, group, seed, n, threads=None):
    out = np.zeros((n, affine_words(curve, group)), dtype=np.uint64)
    threads = threads or min(64, os.cpu_count() or 1)
    _check(test_lib().mnt753_synth_points(curve, group, seed, n, out.ctypes.data_as(C.POINTER(C.c_uint64)), threads), "mnt753_synth_points")
    return out


def synth_scalars(curve, seed, n):
    out = np.zeros((n, 12), dtype=np.uint64)
    _check(lib().mnt753_synth_scalars(curve, seed, n, out.ctypes.data_as(C.POINTER(C.c_uint64))), "mnt753_synth_scalars")
    return out


def synth_expected_msm(curve, group, seed, scalars):
    s, ps = _u64(scalars)
    out = np.zeros(projective_words(curve, group), dtype=np.uint64)
    _check(test_lib().mnt753_synth_expected_msm(curve, group, seed, s.size // 12, ps, out.ctypes.data_as(C.POINTER(C.c_uint64))), "mnt753_synth_expected_msm")
    return out


def test_generator(curve, group):
    """Test hook: the group generator in affine wire form -- the point the pairing levels write for a cancelled pair."""
    out = np.zeros(affine_words(curve, group), dtype=np.uint64)
    _check(test_lib().mnt753_test_generator(curve, group, out.ctypes.data_as(C.POINTER(C.c_uint64))), "mnt753_test_generator")
    return out


def _input_ptr(data, on_device, words, n):
    """-> (pointer, element count, array to keep alive) for a numpy array or, with on_device, a device address"""
    if on_device:
        return C.c_void_p(int(data)), int(n), None
    keep = np.ascontiguousarray(data, dtype=np.uint64)
    return C.c_void_p(keep.ctypes.data), (keep.size // words if n is None else int(n)), keep


def _report(rep):
    return int(rep.n_bad), int(rep.first_bad), int(rep.first_reason)


def check_points(curve, group, affine, on_device=False, n=None, stream=None):
    """mnt753_check_points: canonical coordinates and the curve equation for n affine wire points (a numpy array, or a device address
    with on_device) -> (n_bad, first_bad, reason of first_bad: BAD_*)."""
    ptr, cnt, keep = _input_ptr(affine, on_device, affine_words(curve, group), n)
    rep = CheckReport()
    st = C.c_void_p(int(stream)) if stream else C.c_void_p()
    _check(lib().mnt753_check_points(curve, group, ptr, 1 if on_device else 0, cnt, C.byref(rep), st), "mnt753_check_points")
    return _report(rep)


def check_subgroup(curve, group, affine, on_device=False, n=None, stream=None):
    """mnt753_check_subgroup: check_points plus membership in the subgroup of order r (G2: psi(P) == [t - 1] P per point; G1 has
    cofactor 1) -> (n_bad, first_bad, reason of first_bad: BAD_*, BAD_NOT_IN_SUBGROUP among them)."""
    ptr, cnt, keep = _input_ptr(affine, on_device, affine_words(curve, group), n)
    rep = CheckReport()
    st = C.c_void_p(int(stream)) if stream else C.c_void_p()
    _check(lib().mnt753_check_subgroup(curve, group, ptr, 1 if on_device else 0, cnt, C.byref(rep), st), "mnt753_check_subgroup")
    return _report(rep)


def compressed_words(curve, group):
    return int(lib().mnt753_compressed_words(curve, group))


def compress_points(curve, group, points, on_device=False, n=None, x_out=None, flags_out=None, stream=None):
    """mnt753_compress_points: n affine wire points -> (x [n, compressed_words] uint64, flags [n] uint8: bit 0 the parity of y as an
    integer (G2: of y.c0), bit 1 the identity).  Validates nothing.  on_device: points, x_out and flags_out are device addresses
    (n given) and (x_out, flags_out) come back as they went in."""
    ptr, cnt, keep = _input_ptr(points, on_device, affine_words(curve, group), n)
    st = C.c_void_p(int(stream)) if stream else C.c_void_p()
    if on_device:
        if x_out is None or flags_out is None:
            raise Mnt753Error("compress_points: on_device needs the device addresses x_out and flags_out")
        _check(lib().mnt753_compress_points(curve, group, ptr, 1, cnt, C.c_void_p(int(x_out)), C.c_void_p(int(flags_out)), st), "mnt753_compress_points")
        return x_out, flags_out
    x = np.zeros((cnt, compressed_words(curve, group)), dtype=np.uint64)
    flags = np.zeros(cnt, dtype=np.uint8)
    _check(lib().mnt753_compress_points(curve, group, ptr, 0, cnt, C.c_void_p(x.ctypes.data), C.c_void_p(flags.ctypes.data), st), "mnt753_compress_points")
    return x, flags


def decompress_points(curve, group, x, flags, on_device=False, n=None, out=None, stream=None):
    """mnt753_decompress_points: (x, flags) -> (points [n, affine_words], (n_bad, first_bad, reason of first_bad: BAD_*)); a bad
    point's words are zero, and so are the identity's.  on_device: x, flags and out are device addresses (n given) and out comes back
    in place of the points."""
    ptr, cnt, keep = _input_ptr(x, on_device, compressed_words(curve, group), n)
    rep = CheckReport()
    st = C.c_void_p(int(stream)) if stream else C.c_void_p()
    if on_device:
        if out is None:
            raise Mnt753Error("decompress_points: on_device needs the device address out")
        _check(lib().mnt753_decompress_points(curve, group, ptr, C.c_void_p(int(flags)), 1, cnt, C.c_void_p(int(out)), C.byref(rep), st),
               "mnt753_decompress_points")
        return out, _report(rep)
    fl = np.ascontiguousarray(flags, dtype=np.uint8)
    if fl.size != cnt:
        raise Mnt753Error("decompress_points: one flag byte per point")
    pts = np.zeros((cnt, affine_words(curve, group)), dtype=np.uint64)
    _check(lib().mnt753_decompress_points(curve, group, ptr, C.c_void_p(fl.ctypes.data), 0, cnt, C.c_void_p(pts.ctypes.data), C.byref(rep), st),
           "mnt753_decompress_points")
    return pts, _report(rep)


def points_to_stream(curve, group, x, flags):
    """mnt753_points_to_stream (host only): the packed compressed form -> libff's stream records, bytes"""
    xs = np.ascontiguousarray(x, dtype=np.uint64)
    fl = np.ascontiguousarray(flags, dtype=np.uint8)
    n = fl.size
    if xs.size != n * compressed_words(curve, group):
        raise Mnt753Error("points_to_stream: one flag byte per point")
    ln = C.c_size_t()
    _check(lib().mnt753_points_to_stream(curve, group, C.c_void_p(xs.ctypes.data), C.c_void_p(fl.ctypes.data), n, None, 0, C.byref(ln)),
           "mnt753_points_to_stream")
    buf = np.zeros(max(ln.value, 1), dtype=np.uint8)
    _check(lib().mnt753_points_to_stream(curve, group, C.c_void_p(xs.ctypes.data), C.c_void_p(fl.ctypes.data), n, C.c_void_p(buf.ctypes.data),
                                         ln.value, C.byref(ln)), "mnt753_points_to_stream")
    return buf[:ln.value].tobytes()


def points_from_stream(curve, group, data, n=None):
    """mnt753_points_from_stream (host only): n of libff's stream records (default: as many as data holds) -> (x, flags)"""
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    rec = 8 * compressed_words(curve, group) + 2
    cnt = buf.size // rec if n is None else int(n)
    x = np.zeros((cnt, compressed_words(curve, group)), dtype=np.uint64)
    flags = np.zeros(cnt, dtype=np.uint8)
    _check(lib().mnt753_points_from_stream(curve, group, C.c_void_p(buf.ctypes.data) if buf.size else None, buf.size, cnt,
                                           C.c_void_p(x.ctypes.data), C.c_void_p(flags.ctypes.data)), "mnt753_points_from_stream")
    return x, flags


def test_field_sqrt(curve, deg, elements, window=None):
    """mnt753_test_field_sqrt[_window] (test library): n field elements [n, 12 deg] in wire form -> (roots [n, 12 deg], is_square [n]
    uint8); window = 1, 2, 4 picks the window of the fixed exponent and also returns the kernel's milliseconds."""
    a, pa = _u64(elements)
    n = a.size // (12 * deg)
    out = np.zeros((n, 12 * deg), dtype=np.uint64)
    sq = np.zeros(n, dtype=np.uint8)
    po = out.ctypes.data_as(C.POINTER(C.c_uint64))
    if window is None:
        _check(test_lib().mnt753_test_field_sqrt(curve, deg, pa, n, po, C.c_void_p(sq.ctypes.data)), "mnt753_test_field_sqrt")
        return out, sq
    ms = C.c_float(0)
    _check(test_lib().mnt753_test_field_sqrt_window(curve, deg, window, pa, n, po, C.c_void_p(sq.ctypes.data), C.byref(ms)), "mnt753_test_field_sqrt_window")
    return out, sq, float(ms.value)


def check_scalars(curve, fr, on_device=False, n=None, stream=None):
    """mnt753_check_scalars: every Fr element below r -> (n_bad, first_bad, reason)."""
    ptr, cnt, keep = _input_ptr(fr, on_device, 12, n)
    rep = CheckReport()
    st = C.c_void_p(int(stream)) if stream else C.c_void_p()
    _check(lib().mnt753_check_scalars(curve, ptr, 1 if on_device else 0, cnt, C.byref(rep), st), "mnt753_check_scalars")
    return _report(rep)


def check_products(curve, dev_a, dev_b, dev_c, n, stream=None):
    """mnt753_check_products: a[i] b[i] == c[i] in Fr on three device vectors -> (n_bad, first_bad row, reason)."""
    rep = CheckReport()
    st = C.c_void_p(int(stream)) if stream else C.c_void_p()
    _check(lib().mnt753_check_products(curve, C.c_void_p(int(dev_a)), C.c_void_p(int(dev_b)), C.c_void_p(int(dev_c)), int(n), C.byref(rep), st),
           "mnt753_check_products")
    return _report(rep)


class FixedBase:
    """One base point with its window table on the device (mnt753_fixed_base_*): libff's get_window_table, and batch_exp /
    batch_exp_with_coeff + batch_to_special as `batch_exp`.  window_bits = 0 and tile = 0 leave the width and the scalars per pass to
    the library; both belong to the object."""

    def __init__(self, curve, group, point, window_bits=0, tile=0):
        self.curve, self.group = curve, group
        self._h = C.c_void_p()
        p = np.ascontiguousarray(point, dtype=np.uint64)
        assert p.size == affine_words(curve, group)
        _check(lib().mnt753_fixed_base_create(curve, group, C.c_void_p(p.ctypes.data), int(window_bits), int(tile), C.byref(self._h)),
               "mnt753_fixed_base_create")

    def plan(self):
        t = (C.c_int * 4)()
        _check(lib().mnt753_fixed_base_plan(self._h, t), "mnt753_fixed_base_plan")
        return dict(window_bits=t[0], windows=t[1], inversion_batch=t[2], tile=t[3])

    @property
    def table_bytes(self):
        return int(lib().mnt753_fixed_base_table_bytes(self._h))

    def last_timing(self):
        """HIP-event milliseconds: the table build, and the walk and the normalisation of the last pass of the last batch_exp"""
        t = (C.c_float * 3)()
        _check(lib().mnt753_fixed_base_last_timing(self._h, t), "mnt753_fixed_base_last_timing")
        return dict(table_build_ms=t[0], walk_ms=t[1], normalise_ms=t[2])

    def batch_exp(self, scalars, coeff=None, on_device=False, out_ptr=None, stream=None, n=None):
        """out[i] = (coeff * scalars[i]) * P in affine wire form.  scalars: a numpy array [n, 12], or with on_device a device address
        and n.  Without out_ptr the result comes back as a numpy array [n, affine_words]; with out_ptr (a device address with room for
        n points) it stays on the device and the call returns None."""
        sptr, cnt, keep = _input_ptr(scalars, on_device, 12, n)
        kc = None if coeff is None else np.ascontiguousarray(coeff, dtype=np.uint64)
        assert kc is None or kc.size == 12
        cptr = C.c_void_p(kc.ctypes.data) if kc is not None else C.c_void_p()
        st = C.c_void_p(int(stream)) if stream else C.c_void_p()
        if out_ptr is None:
            out = np.zeros((cnt, affine_words(self.curve, self.group)), dtype=np.uint64)
            optr, out_dev = C.c_void_p(out.ctypes.data if cnt else 0), 0
        else:
            out, optr, out_dev = None, C.c_void_p(int(out_ptr)), 1
        _check(lib().mnt753_batch_exp(self._h, sptr, 1 if on_device else 0, cnt, cptr, optr, out_dev, st), "mnt753_batch_exp")
        return out

    def batch_exp_sparse(self, scalars_ptr, n, out_ptr, coeff=None, stream=None):
        """mnt753_batch_exp_sparse: batch_exp of a device vector through the compaction of its non-zero scalars; both ends on the
        device.  Returns the number of non-zero scalars."""
        kc = None if coeff is None else np.ascontiguousarray(coeff, dtype=np.uint64)
        assert kc is None or kc.size == 12
        cptr = C.c_void_p(kc.ctypes.data) if kc is not None else C.c_void_p()
        st = C.c_void_p(int(stream)) if stream else C.c_void_p()
        cnt = C.c_size_t(0)
        _check(lib().mnt753_batch_exp_sparse(self._h, C.c_void_p(int(scalars_ptr)), int(n), cptr, C.c_void_p(int(out_ptr)), C.byref(cnt), st),
               "mnt753_batch_exp_sparse")
        return int(cnt.value)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().mnt753_fixed_base_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def read_r1cs_file(path):
    """r1cs.bin of oracle/ref_groth16.cpp: u64 num_inputs, m, nc; per matrix a, b, c: u64 row_ptr[nc + 1], u32 col[nnz], Fr coeff[nnz]."""
    raw = np.fromfile(path, dtype=np.uint8)
    num_inputs, m, nc = (int(v) for v in raw[:24].view(np.uint64))
    pos, mats = 24, []
    for _ in range(3):
        rp = raw[pos:pos + 8 * (nc + 1)].view(np.uint64).copy(); pos += 8 * (nc + 1)
        nnz = int(rp[nc])
        col = raw[pos:pos + 4 * nnz].view(np.uint32).copy(); pos += 4 * nnz
        cf = raw[pos:pos + 96 * nnz].view(np.uint64).copy().reshape(nnz, 12); pos += 96 * nnz
        mats.append((rp, col, cf))
    assert pos == raw.size
    return num_inputs, m, nc, mats


class R1cs:
    """Device-resident constraint system (mnt753_r1cs_*): the witness-map front end."""

    def __init__(self, curve, num_inputs, m, nc, mats):
        self.curve, self.num_inputs, self.m, self.nc = curve, num_inputs, m, nc
        self._h = C.c_void_p()
        self._keep = [(np.ascontiguousarray(rp, dtype=np.uint64), np.ascontiguousarray(col, dtype=np.uint32), np.ascontiguousarray(cf, dtype=np.uint64)) for rp, col, cf in mats]
        arr = lambda k: (C.c_void_p * 3)(*[C.c_void_p(t[k].ctypes.data) for t in self._keep])
        _check(lib().mnt753_r1cs_create(curve, num_inputs, m, nc, arr(0), arr(1), arr(2), C.byref(self._h)), "mnt753_r1cs_create")

    @classmethod
    def from_file(cls, curve, path):
        return cls(curve, *read_r1cs_file(path))

    def domain_size(self):
        return int(lib().mnt753_r1cs_domain_size(self._h))

    def evaluate(self, dev_w, dev_ca, dev_cb, dev_cc, out_len, stream=None):
        st = C.c_void_p(int(stream)) if stream else C.c_void_p()
        _check(lib().mnt753_r1cs_evaluate(self._h, C.c_void_p(int(dev_w)), C.c_void_p(int(dev_ca)), C.c_void_p(int(dev_cb)), C.c_void_p(int(dev_cc)),
                                          int(out_len), st), "mnt753_r1cs_evaluate")

    def check(self, dev_w, stream=None):
        """mnt753_r1cs_check: does the assignment at dev_w (m + 1 elements) satisfy the system -> (n_bad, first bad constraint row, reason)."""
        rep = CheckReport()
        st = C.c_void_p(int(stream)) if stream else C.c_void_p()
        _check(lib().mnt753_r1cs_check(self._h, C.c_void_p(int(dev_w)), C.byref(rep), st), "mnt753_r1cs_check")
        return _report(rep)

    def swap_ab_if_beneficial(self):
        """swap_AB_if_beneficial of the reference (mnt753_r1cs_swap_ab_if_beneficial): a and b change roles inside the device object if b
        touches strictly more variables.  Returns True if this call exchanged them; `swapped` tells how the system stands."""
        flag = C.c_int(0)
        _check(lib().mnt753_r1cs_swap_ab_if_beneficial(self._h, C.byref(flag)), "mnt753_r1cs_swap_ab_if_beneficial")
        return bool(flag.value)

    @property
    def swapped(self):
        """True if a and b stand exchanged relative to the matrices the object was created from"""
        return bool(lib().mnt753_r1cs_is_swapped(self._h))

    def host_matrices(self):
        """the matrices as the device object now holds them: (row_ptr, col, coeff) of a, b, c, with a and b exchanged if `swapped`"""
        a, b, c = self._keep
        return [b, a, c] if self.swapped else [a, b, c]

    def qap_plan(self):
        """mnt753_r1cs_qap_plan: how qap_at cuts the columns (builds the column-major view if no call has yet)."""
        p = QapPlan()
        _check(lib().mnt753_r1cs_qap_plan(self._h, C.byref(p)), "mnt753_r1cs_qap_plan")
        return dict(chunk_terms=int(p.chunk_terms), terms=int(p.terms), work_items=int(p.work_items), split_columns=int(p.split_columns),
                    longest_column=int(p.longest_column), transpose_bytes=int(p.transpose_bytes), partial_bytes=int(p.partial_bytes))

    def qap_at(self, domain, t, out=None, stream=None):
        """r1cs_to_qap_instance_map_with_evaluation at t on `domain` (mnt753_r1cs_qap_at).  out: device addresses (At, Bt, Ct, Ht) with
        room for m + 1, m + 1, m + 1 and domain.m + 1 elements, or None for four new DeviceBuffers.  Returns (At, Bt, Ct, Ht, Zt): the
        four device buffers (or the addresses given) and Zt as 12 uint64 on the host; the vectors are complete when `stream` has run."""
        k, pk = _fr_elem(t)
        st = C.c_void_p(int(stream)) if stream else C.c_void_p()
        if out is None:
            bufs = [DeviceBuffer(96 * (self.m + 1)) for _ in range(3)] + [DeviceBuffer(96 * (domain.m + 1))]
            ptrs = [b.ptr for b in bufs]
        else:
            bufs = list(out)
            ptrs = [C.c_void_p(int(p)) for p in out]
        zt = np.zeros(12, dtype=np.uint64)
        _check(lib().mnt753_r1cs_qap_at(self._h, domain._h, pk, ptrs[0], ptrs[1], ptrs[2], ptrs[3], zt.ctypes.data_as(C.POINTER(C.c_uint64)), st),
               "mnt753_r1cs_qap_at")
        return bufs[0], bufs[1], bufs[2], bufs[3], zt

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().mnt753_r1cs_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def write_r1cs_file(path, num_inputs, m, nc, mats):
    """the inverse of read_r1cs_file"""
    with open(path, "wb") as f:
        f.write(np.array([num_inputs, m, nc], dtype="<u8").tobytes())
        for rp, col, cf in mats:
            f.write(np.ascontiguousarray(rp, dtype="<u8").tobytes())
            f.write(np.ascontiguousarray(col, dtype="<u4").tobytes())
            f.write(np.ascontiguousarray(cf, dtype="<u8").tobytes())


def group_generator(curve, group):
    """G1::one() / G2::one() of the curve in the affine wire format (mnt753_group_generator)"""
    out = np.zeros(affine_words(curve, group), dtype=np.uint64)
    _check(lib().mnt753_group_generator(curve, group, out.ctypes.data_as(C.POINTER(C.c_uint64))), "mnt753_group_generator")
    return out


def compact_nonzero(scalars_ptr, n, compact_ptr=None, index_ptr=None, stream=None):
    """mnt753_compact_nonzero on a device vector of n Fr elements -> the number of non-zero elements; with compact_ptr / index_ptr
    (device addresses with room for n elements / n uint32) the compacted elements and their indices are written too."""
    st = C.c_void_p(int(stream)) if stream else C.c_void_p()
    cnt = C.c_size_t(0)
    cp = C.c_void_p(int(compact_ptr)) if compact_ptr else C.c_void_p()
    ip = C.c_void_p(int(index_ptr)) if index_ptr else C.c_void_p()
    _check(lib().mnt753_compact_nonzero(C.c_void_p(int(scalars_ptr)), int(n), cp, ip, C.byref(cnt), st), "mnt753_compact_nonzero")
    return int(cnt.value)


def scatter_rows(rows_ptr, index_ptr, count, row_words, out_ptr, n, stream=None):
    """mnt753_scatter_rows: out[index[j]] = rows[j], zero words in every other of the n rows of out"""
    st = C.c_void_p(int(stream)) if stream else C.c_void_p()
    _check(lib().mnt753_scatter_rows(C.c_void_p(int(rows_ptr)), C.c_void_p(int(index_ptr)), int(count), int(row_words), C.c_void_p(int(out_ptr)), int(n), st),
           "mnt753_scatter_rows")


def keygen_combine(curve, at_ptr, bt_ptr, ct_ptr, n, num_inputs, beta, alpha, dinv, out_ptr, stream=None):
    """mnt753_keygen_combine: out[i] = (beta At[i] + alpha Bt[i] + Ct[i]) c_i, c_i = 1 for i <= num_inputs and dinv above"""
    st = C.c_void_p(int(stream)) if stream else C.c_void_p()
    (kb, pb), (ka, pa), (kd, pd) = _fr_elem(beta), _fr_elem(alpha), _fr_elem(dinv)
    _check(lib().mnt753_keygen_combine(curve, C.c_void_p(int(at_ptr)), C.c_void_p(int(bt_ptr)), C.c_void_p(int(ct_ptr)), int(n), int(num_inputs),
                                       pb, pa, pd, C.c_void_p(int(out_ptr)), st), "mnt753_keygen_combine")


class GeneratedKey:
    """A Groth16 key as mnt753_groth16_generate makes it.  The query vectors stay on the device (`buffers`: DeviceBuffers named
    A, B1, B2, L, H, ABC); `bases(which)` makes a BaseSet of one without a copy through the host; `write(dir)` writes the files of
    `main_hip generate`.  `non_zero_at` / `non_zero_bt` are the reference's query densities, `swapped` says whether this call's
    swap_AB_if_beneficial exchanged a and b (the system the key is for is `r1cs_matrices`, which write() puts into r1cs.bin).
    from_host() builds the same object around numpy arrays, for writing a key that is already in host memory."""

    QUERIES = (("A", G1), ("B1", G1), ("B2", G2), ("L", G1), ("H", G1), ("ABC", G1))

    def __init__(self, curve, num_inputs, num_variables, num_constraints, domain_size, counts, singles, r1cs_matrices, buffers=None, host=None,
                 non_zero_at=None, non_zero_bt=None, swapped=False):
        self.curve, self.num_inputs, self.num_variables, self.num_constraints = curve, int(num_inputs), int(num_variables), int(num_constraints)
        self.domain_size = int(domain_size)
        self.counts = dict(counts)              # elements of each query
        self.singles = dict(singles)            # alpha_g1, beta_g1, beta_g2, delta_g1, delta_g2: numpy words
        self.r1cs_matrices = r1cs_matrices
        self.buffers, self._host = buffers or {}, dict(host or {})
        self.non_zero_at, self.non_zero_bt, self.swapped = non_zero_at, non_zero_bt, bool(swapped)

    @classmethod
    def from_host(cls, curve, num_inputs, num_variables, num_constraints, domain_size, queries, singles, r1cs_matrices, **kw):
        """queries: {"A": words, ...} numpy arrays in the affine wire format"""
        host = {k: np.ascontiguousarray(v, dtype=np.uint64).reshape(-1) for k, v in queries.items()}
        counts = {k: host[k].size // affine_words(curve, g) for k, g in cls.QUERIES}
        return cls(curve, num_inputs, num_variables, num_constraints, domain_size, counts, singles, r1cs_matrices, host=host, **kw)

    def query(self, which):
        """the words of one query in host memory (copied from the device on first use)"""
        if which not in self._host:
            group = dict(self.QUERIES)[which]
            n = self.counts[which] * affine_words(self.curve, group)
            self._host[which] = self.buffers[which].to_numpy()[:n] if n else np.zeros(0, dtype=np.uint64)
        return self._host[which]

    def bases(self, which):
        """a BaseSet over the query `which` ("A", "B1", "B2", "L", "H" or "ABC") as it lies on the device"""
        group = dict(self.QUERIES)[which]
        return BaseSet(self.curve, group, self.buffers[which].ptr.value, on_device=True, n=self.counts[which])

    def verification_key(self):
        """the VerificationKey of this key: alpha_g1, beta_g2, delta_g2 and the ABC query (copied from the device)"""
        s = self.singles
        return VerificationKey(self.curve, s["alpha_g1"], s["beta_g2"], s["delta_g2"], self.query("ABC"))

    def write(self, out_dir):
        """params.bin (the challenge layout of generate_parameters.cpp:60-85: u64 d = domain size - 1, u64 m, then A | B1 | B2 | L | H),
        keys.bin (alpha_g1 | beta_g1 | beta_g2 | delta_g1 | delta_g2, what `main_hip complete` reads), vk_elements.bin (alpha_g1 |
        beta_g2 | delta_g2 | ABC_g1: a verification key without its GT element, which needs a pairing) and r1cs.bin (the system the
        key is for: a and b exchanged if the swap fired)."""
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "params.bin"), "wb") as f:
            f.write(np.array([self.domain_size - 1, self.num_variables], dtype="<u8").tobytes())
            for which in ("A", "B1", "B2", "L", "H"):
                f.write(self.query(which).astype("<u8").tobytes())
        s = self.singles
        with open(os.path.join(out_dir, "keys.bin"), "wb") as f:
            for k in ("alpha_g1", "beta_g1", "beta_g2", "delta_g1", "delta_g2"):
                f.write(np.ascontiguousarray(s[k], dtype="<u8").tobytes())
        with open(os.path.join(out_dir, "vk_elements.bin"), "wb") as f:
            for k in ("alpha_g1", "beta_g2", "delta_g2"):
                f.write(np.ascontiguousarray(s[k], dtype="<u8").tobytes())
            f.write(self.query("ABC").astype("<u8").tobytes())
        write_r1cs_file(os.path.join(out_dir, "r1cs.bin"), self.num_inputs, self.num_variables, self.num_constraints, self.r1cs_matrices)

    def close(self):
        for b in self.buffers.values():
            b.close()
        self.buffers = {}


def generate(r1cs, domain, t, alpha, beta, delta, g1_generator, g1_window_bits=0, g2_window_bits=0, g1_tile=0, g2_tile=0,
             sparse_g1=True, sparse_g2=True, stream=None):
    """mnt753_groth16_generate: the reference's Groth16 generator with its randomness as arguments -- t, alpha, beta, delta (12 uint64
    each, wire form) and the G1 generator (24 uint64, affine).  The system object is swapped in place if the reference's rule says so.
    Window widths and tiles of 0 leave the two tables to the library; sparse_g1 / sparse_g2 say whether the G1 queries of At and Bt /
    the G2 query of Bt go through the compaction of their non-zero scalars (both do by default).  Returns a GeneratedKey."""
    sizes = KeygenSizes()
    _check(lib().mnt753_groth16_sizes(r1cs._h, domain._h, C.byref(sizes)), "mnt753_groth16_sizes")
    counts = {"A": sizes.a_query, "B1": sizes.b_g1_query, "B2": sizes.b_g2_query, "L": sizes.l_query, "H": sizes.h_query, "ABC": sizes.abc_g1}
    curve = r1cs.curve
    bufs = {k: DeviceBuffer(8 * affine_words(curve, g) * max(int(counts[k]), 1)) for k, g in GeneratedKey.QUERIES}
    singles = {k: np.zeros(affine_words(curve, g), dtype=np.uint64)
               for k, g in (("alpha_g1", G1), ("beta_g1", G1), ("beta_g2", G2), ("delta_g1", G1), ("delta_g2", G2))}
    out = KeygenOut(*[bufs[k].ptr.value for k, _ in GeneratedKey.QUERIES],
                    *[singles[k].ctypes.data for k in ("alpha_g1", "beta_g1", "beta_g2", "delta_g1", "delta_g2")])
    out.dev_l_query = bufs["L"].ptr.value
    opts = KeygenOpts(int(g1_window_bits), int(g2_window_bits), int(g1_tile), int(g2_tile),
                      (0 if sparse_g1 else KEYGEN_DENSE_G1) | (0 if sparse_g2 else KEYGEN_DENSE_G2), 0)
    rep = KeygenReport()
    (kt, pt), (ka, pa), (kb, pb), (kd, pd) = _fr_elem(t), _fr_elem(alpha), _fr_elem(beta), _fr_elem(delta)
    g = np.ascontiguousarray(g1_generator, dtype=np.uint64).reshape(-1)
    assert g.size == 24
    st = C.c_void_p(int(stream)) if stream else C.c_void_p()
    rc = lib().mnt753_groth16_generate(r1cs._h, domain._h, pt, pa, pb, pd, g.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(opts), C.byref(out),
                                       C.byref(rep), st)
    if rc != 0:
        for b in bufs.values():
            b.close()
        _check(rc, "mnt753_groth16_generate")
    return GeneratedKey(curve, r1cs.num_inputs, r1cs.m, r1cs.nc, domain.m, counts, singles, r1cs.host_matrices(), buffers=bufs,
                        non_zero_at=int(rep.non_zero_at), non_zero_bt=int(rep.non_zero_bt), swapped=bool(rep.swapped))


def test_field_op(mod, op, a, b=None):
    """Test hook: the device field layer element-wise on wire-form elements (see include/mnt753_hip.h)."""
    a, pa = _u64(a)
    b, pb = _u64(a if b is None else b)
    out = np.zeros_like(a)
    _check(test_lib().mnt753_test_field_op(mod, op, pa, pb, a.size // 12, out.ctypes.data_as(C.POINTER(C.c_uint64))), "mnt753_test_field_op")
    return out


FIELD_RAW_IN_WORDS, FIELD_RAW_OUT_WORDS = 6 * 27, 2 * 27 + 1


def test_field_raw(mod, op, records, k=0):
    """Test hook: one device field primitive on raw limbs (csrc/field_raw_ops.hip.h).  records: uint32 array of shape (n, 162)
    (6 operands x 27 limbs); returns (n, 55): two results of 27 limbs and a flag word."""
    rec = np.ascontiguousarray(records, dtype=np.uint32).reshape(-1, FIELD_RAW_IN_WORDS)
    out = np.zeros((rec.shape[0], FIELD_RAW_OUT_WORDS), dtype=np.uint32)
    u32p = C.POINTER(C.c_uint32)
    _check(test_lib().mnt753_test_field_raw(mod, op, rec.ctypes.data_as(u32p), rec.shape[0], k, out.ctypes.data_as(u32p)), "mnt753_test_field_raw")
    return out


def test_ext_raw(curve, split, op, a, b=None):
    """Test hook: Fq2 (MNT4753) / Fq3 (MNT6753) on raw device components; a, b: uint32 arrays of shape (n, deg * 27)."""
    deg = 2 if curve == 0 else 3
    a = np.ascontiguousarray(a, dtype=np.uint32).reshape(-1, deg * 27)
    b = a if b is None else np.ascontiguousarray(b, dtype=np.uint32).reshape(-1, deg * 27)
    out = np.zeros_like(a)
    u32p = C.POINTER(C.c_uint32)
    _check(test_lib().mnt753_test_ext_raw(curve, int(split), op, a.ctypes.data_as(u32p), b.ctypes.data_as(u32p), a.shape[0],
                                          out.ctypes.data_as(u32p)), "mnt753_test_ext_raw")
    return out


def test_ext_op(curve, split, op, a, b=None):
    """Test hook: Fq2 (MNT4753) / Fq3 (MNT6753) on the device, element-wise; split = the lane-split form of the G2 kernels."""
    a, pa = _u64(a)
    b, pb = _u64(a if b is None else b)
    out = np.zeros_like(a)
    words = 12 * (2 if curve == 0 else 3)
    _check(test_lib().mnt753_test_ext_op(curve, int(split), op, pa, pb, a.size // words, out.ctypes.data_as(C.POINTER(C.c_uint64))), "mnt753_test_ext_op")
    return out


def test_point_op(curve, group, split, op, p, q=None):
    """Test hook: one form of the device group law on projective wire points (see include/mnt753_hip.h)."""
    p, pp = _u64(p)
    q, pq = _u64(p if q is None else q)
    out = np.zeros_like(p)
    _check(test_lib().mnt753_test_point_op(curve, group, int(split), op, pp, pq, p.size // projective_words(curve, group),
                                      out.ctypes.data_as(C.POINTER(C.c_uint64))), "mnt753_test_point_op")
    return out


test_generator.__test__ = False
test_field_raw.__test__ = False
test_ext_raw.__test__ = False
test_ext_op.__test__ = False
test_point_op.__test__ = False


def mont_one(curve):
    """Fr element 1 in wire (Montgomery) form: R mod r."""
    r = [0x0001c4c62d92c41110229022eee2cdadb7f997505b8fafed5eb7e8f96c97d87307fdb925e8a0ed8d99d124d9a15af79db26c5c28c859a99b3eebca9429212636b9dff97634993aa4d6c381bc3f0057974ea099170fa13a4fd90776e240000001,
         0x0001c4c62d92c41110229022eee2cdadb7f997505b8fafed5eb7e8f96c97d87307fdb925e8a0ed8d99d124d9a15af79db117e776f218059db80f0da5cb537e38685acce9767254a4638810719ac425f0e39d54522cdd119f5e9063de245e8001][curve]
    v = (1 << 768) % r
    return np.array([(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(12)], dtype=np.uint64)


# ---- the pairing and Groth16 verification -----------------------------------------------------------------------------------------
def gt_words(curve):
    return int(lib().mnt753_gt_words(curve))


def pairing(curve, P, Q, on_device=False, n=None, out=None, stream=None):
    """mnt753_pairing: e(P[i], Q[i]) for affine wire-format points -> numpy words [n, gt_words] (host arrays), or into the device
    address `out` with on_device.  A malformed point raises Mnt753Error; the identity in either argument gives GT one."""
    p1, cnt, keep1 = _input_ptr(P, on_device, 24, n)
    p2, cnt2, keep2 = _input_ptr(Q, on_device, affine_words(curve, G2), n)
    if cnt != cnt2:
        raise Mnt753Error("pairing: as many G1 as G2 points")
    st = C.c_void_p(int(stream)) if stream else C.c_void_p()
    if on_device:
        _check(lib().mnt753_pairing(curve, p1, p2, cnt, 1, C.c_void_p(int(out)), st), "mnt753_pairing")
        return None
    res = np.zeros((cnt, gt_words(curve)), dtype=np.uint64)
    _check(lib().mnt753_pairing(curve, p1, p2, cnt, 0, C.c_void_p(res.ctypes.data), st), "mnt753_pairing")
    return res


class VerificationKey:
    """mnt753_vk: a Groth16 verification key on the device.  alpha_g1, beta_g2, delta_g2: affine wire words; abc_g1: num_inputs + 1
    G1 points.  from_elements() takes the contents of `generate`'s vk_elements.bin."""

    def __init__(self, curve, alpha_g1, beta_g2, delta_g2, abc_g1):
        self.curve = curve
        a, pa = _u64(alpha_g1)
        b, pb = _u64(beta_g2)
        d, pd = _u64(delta_g2)
        abc, pabc = _u64(np.asarray(abc_g1).reshape(-1))
        if a.size != 24 or b.size != affine_words(curve, G2) or d.size != b.size or abc.size < 24 or abc.size % 24:
            raise Mnt753Error("VerificationKey: element sizes do not fit the curve")
        self.num_inputs = abc.size // 24 - 1
        self._g2 = np.concatenate([b, d])          # beta_g2 | delta_g2, for check_subgroup()
        self._h = C.c_void_p()
        _check(lib().mnt753_vk_create(curve, pa, pb, pd, pabc, self.num_inputs, C.byref(self._h)), "mnt753_vk_create")

    @classmethod
    def from_elements(cls, curve, words):
        """words: alpha_g1 | beta_g2 | delta_g2 | ABC_g1 (vk_elements.bin)"""
        w = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1)
        w2 = affine_words(curve, G2)
        return cls(curve, w[:24], w[24:24 + w2], w[24 + w2:24 + 2 * w2], w[24 + 2 * w2:])

    def gt(self):
        out = np.zeros(gt_words(self.curve), dtype=np.uint64)
        _check(lib().mnt753_vk_gt(self._h, out.ctypes.data_as(C.POINTER(C.c_uint64))), "mnt753_vk_gt")
        return out

    def coefficient_bytes(self):
        """device memory of the stored Miller-loop coefficients of G2::one() and delta_g2"""
        return int(lib().mnt753_vk_coefficient_bytes(self._h))

    def set_workspace_cap(self, nbytes):
        """bytes a verify() call may allocate for a chunk of proofs (0: the default chunk of 2^16 proofs)"""
        _check(lib().mnt753_vk_set_workspace_cap(self._h, int(nbytes)), "mnt753_vk_set_workspace_cap")

    def serialize(self):
        """the bytes of the reference's vk.txt"""
        ln = C.c_size_t()
        _check(lib().mnt753_vk_serialize(self._h, None, 0, C.byref(ln)), "mnt753_vk_serialize")
        buf = (C.c_uint8 * ln.value)()
        _check(lib().mnt753_vk_serialize(self._h, C.cast(buf, C.c_void_p), ln.value, C.byref(ln)), "mnt753_vk_serialize")
        return bytes(buf)

    def accumulate(self, inputs):
        """inputs: [n, num_inputs, 12] Fr words -> [n, 24]: ABC[0] + sum_j inputs[i][j] ABC[j + 1]"""
        x, px = _u64(np.asarray(inputs).reshape(-1))
        n = x.size // (12 * self.num_inputs) if self.num_inputs else int(np.asarray(inputs).shape[0])
        out = np.zeros((n, 24), dtype=np.uint64)
        _check(lib().mnt753_vk_accumulate(self._h, px, n, out.ctypes.data_as(C.POINTER(C.c_uint64))), "mnt753_vk_accumulate")
        return out

    def prepare_inputs(self, window_bits=0, max_table_bytes=0):
        """mnt753_vk_prepare_inputs: one signed-digit window table per ABC point on the device; accumulate(),
        verify(), verify_compressed() and verify_folded() then walk the tables -- the same results, W = ceil(754 / w) additions per
        input.  window_bits 0: the widest width in 2 .. 16 whose tables fit max_table_bytes (0: 256 MiB).  Opt-in: nothing prepares a
        key by itself.  A refusal (Mnt753Error) leaves the key as it was.  Returns input_plan()."""
        _check(lib().mnt753_vk_prepare_inputs(self._h, int(window_bits), int(max_table_bytes)), "mnt753_vk_prepare_inputs")
        return self.input_plan()

    def input_plan(self, n=1):
        """mnt753_vk_input_plan for a chunk of n proofs -> dict: prepared, window_bits, windows, inputs_per_lane, table_bytes"""
        out = VkInputPlan()
        _check(lib().mnt753_vk_input_plan(self._h, int(n), C.byref(out)), "mnt753_vk_input_plan")
        return {"prepared": bool(out.prepared), "window_bits": int(out.window_bits), "windows": int(out.windows),
                "inputs_per_lane": int(out.inputs_per_lane), "table_bytes": int(out.table_bytes)}

    def release_inputs(self):
        """mnt753_vk_release_inputs: frees the input tables; the key is back on the path of an unprepared key"""
        _check(lib().mnt753_vk_release_inputs(self._h), "mnt753_vk_release_inputs")

    def test_force_inputs_per_lane(self, inputs_per_lane):
        """mnt753_test_vk_force_inputs_per_lane (test library): scalars per lane of the walk of every later call (0: the host's choice)"""
        _check(test_lib().mnt753_test_vk_force_inputs_per_lane(self._h, int(inputs_per_lane)), "mnt753_test_vk_force_inputs_per_lane")

    def test_inputs_last_timing(self):
        """mnt753_test_vk_inputs_last_timing (test library): milliseconds of the walk, of the segment sum with the normalisation (last
        chunk) and of the last build of the tables"""
        out = (C.c_float * 3)()
        _check(test_lib().mnt753_test_vk_inputs_last_timing(self._h, out), "mnt753_test_vk_inputs_last_timing")
        return [float(v) for v in out]

    def test_set_gt(self, words):
        """mnt753_test_vk_set_gt (test library): overwrites the key's e(alpha_g1, beta_g2), on the device and on the host"""
        g, pg = _u64(np.asarray(words).reshape(-1))
        if g.size != gt_words(self.curve):
            raise Mnt753Error("test_set_gt: gt_words(curve) words")
        _check(test_lib().mnt753_test_vk_set_gt(self._h, pg), "mnt753_test_vk_set_gt")

    def check_subgroup(self):
        """beta_g2 and delta_g2 of the key through check_subgroup -> (n_bad, first_bad: 0 = beta_g2, 1 = delta_g2, reason).  The key's
        constructor (mnt753_vk_create) does not test membership itself."""
        return check_subgroup(self.curve, G2, self._g2)

    def verify(self, proofs, inputs, on_device=False, n=None, stream=None, check_subgroup=False, fold=False):
        """proofs: n x (A | B | C) affine wire words, inputs: n x num_inputs Fr (numpy arrays, or device addresses with on_device and n)
        -> numpy uint8 verdicts [n]: 0 accepted, 1 malformed, 2 the pairing check failed; with check_subgroup also 3: B is not in the
        order-r subgroup of the twist (mnt753_groth16_verify_ex with MNT753_VERIFY_CHECK_SUBGROUP).
        fold: verify_folded() with fresh coefficients first -- an accepted batch is all zeros after one final exponentiation -- and, if
        the fold rejects, the per-proof pass with check_subgroup, which names the proofs."""
        if fold:
            accepted, status = self.verify_folded(proofs, inputs, on_device=on_device, n=n, stream=stream)
            if accepted:
                return status
            return self.verify(proofs, inputs, on_device=on_device, n=n, stream=stream, check_subgroup=True)
        pw = 48 + affine_words(self.curve, G2)
        pp, cnt, keep1 = _input_ptr(proofs, on_device, pw, n)
        if self.num_inputs:
            pi, cnt2, keep2 = _input_ptr(inputs, on_device, 12 * self.num_inputs, n)
            if cnt2 != cnt:
                raise Mnt753Error("verify: one row of inputs per proof")
        else:
            pi = C.c_void_p()
        verdicts = np.zeros(cnt, dtype=np.uint8)
        st = C.c_void_p(int(stream)) if stream else C.c_void_p()
        if check_subgroup:
            rc = lib().mnt753_groth16_verify_ex(self._h, pp, pi, cnt, 1 if on_device else 0, VERIFY_CHECK_SUBGROUP, C.c_void_p(verdicts.ctypes.data), st)
        else:
            rc = lib().mnt753_groth16_verify(self._h, pp, pi, cnt, 1 if on_device else 0, C.c_void_p(verdicts.ctypes.data), st)
        if rc < 0:
            _check(rc, "mnt753_groth16_verify")
        return verdicts

    def verify_compressed(self, x, flags, inputs, check_subgroup=False, on_device=False, n=None, stream=None):
        """mnt753_groth16_verify_compressed.  x: n x (x_A | x_B | x_C) words, flags: n x 3 bytes (compress_points of A, B, C), inputs
        as for verify() (numpy arrays, or device addresses with on_device and n) -> verdicts as verify(); 1 (malformed) also covers a
        point that does not decompress and an identity flag."""
        xw = 24 + compressed_words(self.curve, G2)
        px, cnt, keep1 = _input_ptr(x, on_device, xw, n)
        if on_device:
            pf, keep3 = C.c_void_p(int(flags)), None
        else:
            keep3 = np.ascontiguousarray(flags, dtype=np.uint8)
            if keep3.size != 3 * cnt:
                raise Mnt753Error("verify_compressed: three flag bytes per proof")
            pf = C.c_void_p(keep3.ctypes.data)
        if self.num_inputs:
            pi, cnt2, keep2 = _input_ptr(inputs, on_device, 12 * self.num_inputs, n)
            if cnt2 != cnt:
                raise Mnt753Error("verify_compressed: one row of inputs per proof")
        else:
            pi = C.c_void_p()
        verdicts = np.zeros(cnt, dtype=np.uint8)
        st = C.c_void_p(int(stream)) if stream else C.c_void_p()
        rc = lib().mnt753_groth16_verify_compressed(self._h, px, pf, pi, cnt, 1 if on_device else 0, VERIFY_CHECK_SUBGROUP if check_subgroup else 0,
                                                    C.c_void_p(verdicts.ctypes.data), st)
        if rc < 0:
            _check(rc, "mnt753_groth16_verify_compressed")
        return verdicts

    def _fold_args(self, proofs, inputs, coefficients, on_device, n):
        pw = 48 + affine_words(self.curve, G2)
        pp, cnt, keep1 = _input_ptr(proofs, on_device, pw, n)
        if self.num_inputs:
            pi, cnt2, keep2 = _input_ptr(inputs, on_device, 12 * self.num_inputs, n)
            if cnt2 != cnt:
                raise Mnt753Error("verify_folded: one row of inputs per proof")
        else:
            pi, keep2 = C.c_void_p(), None
        if coefficients is None:
            import secrets
            coefficients = [secrets.randbelow(2 ** 128 - 1) + 1 for _ in range(cnt)]
        if isinstance(coefficients, np.ndarray) and coefficients.dtype == np.uint64:
            co = np.ascontiguousarray(coefficients).reshape(-1)
        else:
            co = np.array([(int(v) >> (64 * k)) & (2 ** 64 - 1) for v in coefficients for k in range(2)], dtype=np.uint64)
        if co.size != 2 * cnt:
            raise Mnt753Error("verify_folded: one 128-bit coefficient per proof")
        return pp, pi, cnt, co, (keep1, keep2)

    def verify_folded(self, proofs, inputs, coefficients=None, on_device=False, n=None, stream=None):
        """mnt753_groth16_verify_folded: the batch under ONE final exponentiation -> (accepted, status [n]:
        0, 1 malformed, 3 B not in the subgroup).  coefficients: n integers 0 < rho_i < 2^128 (or [n, 2] uint64 words); None draws them
        from `secrets` -- they must not be predictable by whoever made the proofs.  A rejected batch does not name the wrong proof:
        verify(.., fold=True) falls back to the per-proof pass."""
        pp, pi, cnt, co, keep = self._fold_args(proofs, inputs, coefficients, on_device, n)
        status = np.zeros(cnt, dtype=np.uint8)
        accepted = C.c_int(0)
        st = C.c_void_p(int(stream)) if stream else C.c_void_p()
        _check(lib().mnt753_groth16_verify_folded(self._h, pp, pi, cnt, 1 if on_device else 0, co.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                  C.c_void_p(status.ctypes.data), C.byref(accepted), st), "mnt753_groth16_verify_folded")
        return bool(accepted.value), status

    def test_fold_parts(self, proofs, inputs, coefficients):
        """mnt753_test_fold_parts (test library) on host arrays -> dict: f (the unreduced product), s, t (affine wire form), rho (Fr
        wire form), status, accepted"""
        pp, pi, cnt, co, keep = self._fold_args(proofs, inputs, coefficients, False, None)
        u64p = C.POINTER(C.c_uint64)
        f, s, t, rho = (np.zeros(k, dtype=np.uint64) for k in (gt_words(self.curve), 24, 24, 12))
        status = np.zeros(cnt, dtype=np.uint8)
        accepted = C.c_int(0)
        _check(test_lib().mnt753_test_fold_parts(self._h, C.cast(pp, u64p), C.cast(pi, u64p), cnt, co.ctypes.data_as(u64p), f.ctypes.data_as(u64p),
                                                 s.ctypes.data_as(u64p), t.ctypes.data_as(u64p), rho.ctypes.data_as(u64p),
                                                 C.c_void_p(status.ctypes.data), C.byref(accepted)), "mnt753_test_fold_parts")
        return {"f": f, "s": s, "t": t, "rho": rho, "status": status, "accepted": bool(accepted.value)}

    def verify_folded_locate(self, proofs, inputs, coefficients=None, on_device=False, n=None, stream=None):
        """mnt753_groth16_verify_folded_locate: the fold with one tail per segment of fold_segment_proofs(curve) proofs (DESIGN.md
        section 4.18) -> (verdicts [n] as verify(.., check_subgroup=True), report dict: segments, segments_rejected, proofs_rechecked,
        ms_scale, ms_miller, ms_tails, ms_recheck).  Only the rejected segments pay the per-proof pass.  coefficients as for
        verify_folded(): None draws them from `secrets`."""
        pp, pi, cnt, co, keep = self._fold_args(proofs, inputs, coefficients, on_device, n)
        verdicts = np.zeros(cnt, dtype=np.uint8)
        rep = FoldLocateReport()
        st = C.c_void_p(int(stream)) if stream else C.c_void_p()
        rc = lib().mnt753_groth16_verify_folded_locate(self._h, pp, pi, cnt, 1 if on_device else 0, co.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                       C.c_void_p(verdicts.ctypes.data), C.byref(rep), st)
        if rc < 0:
            _check(rc, "mnt753_groth16_verify_folded_locate")
        return verdicts, rep.as_dict()

    def test_fold_segment_parts(self, proofs, inputs, coefficients):
        """mnt753_test_fold_segment_parts (test library) on host arrays -> dict, one row per segment: f [segments, gt_words] (the
        unreduced products), s, t [segments, 24] (affine wire form), rho [segments, 12] (Fr wire form), accepted [segments]; status
        and verdicts [n]; report"""
        pp, pi, cnt, co, keep = self._fold_args(proofs, inputs, coefficients, False, None)
        u64p = C.POINTER(C.c_uint64)
        g = fold_segment_proofs(self.curve)
        segs = (cnt + g - 1) // g
        f, s, t, rho = (np.zeros((segs, k), dtype=np.uint64) for k in (gt_words(self.curve), 24, 24, 12))
        accepted = np.zeros(segs, dtype=np.uint8)
        status = np.zeros(cnt, dtype=np.uint8)
        verdicts = np.zeros(cnt, dtype=np.uint8)
        rep = FoldLocateReport()
        rc = test_lib().mnt753_test_fold_segment_parts(self._h, C.cast(pp, u64p), C.cast(pi, u64p), cnt, co.ctypes.data_as(u64p), f.ctypes.data_as(u64p),
                                                       s.ctypes.data_as(u64p), t.ctypes.data_as(u64p), rho.ctypes.data_as(u64p),
                                                       C.c_void_p(accepted.ctypes.data), C.c_void_p(status.ctypes.data),
                                                       C.c_void_p(verdicts.ctypes.data), C.byref(rep))
        if rc < 0:
            _check(rc, "mnt753_test_fold_segment_parts")
        return {"f": f, "s": s, "t": t, "rho": rho, "accepted": accepted, "status": status, "verdicts": verdicts, "report": rep.as_dict()}

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().mnt753_vk_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def fold_segment_proofs(curve):
    """mnt753_fold_segment_proofs: proofs per segment of verify_folded_locate() -- 128 (MNT4753) or 84 (MNT6753)"""
    return int(lib().mnt753_fold_segment_proofs(curve))


def test_fold_locate_last_chunks():
    """mnt753_test_fold_locate_last_chunks (test library): chunks the last verify_folded_locate / test_fold_segment_parts ran"""
    return int(test_lib().mnt753_test_fold_locate_last_chunks())


def test_fold_last_timing():
    """mnt753_test_fold_last_timing (test library): milliseconds of the scale, Miller-and-fold and tail stages of the last folded call"""
    out = (C.c_float * 3)()
    _check(test_lib().mnt753_test_fold_last_timing(out), "mnt753_test_fold_last_timing")
    return [float(v) for v in out]


def test_tower_op(curve, split, op, a, b=None):
    """mnt753_test_tower_op (test library): a, b [n, gt_words] -> [n, gt_words]"""
    a, pa = _u64(a)
    b, pb = _u64(a if b is None else b)
    out = np.zeros_like(a)
    n = a.size // gt_words(curve)
    _check(test_lib().mnt753_test_tower_op(curve, split, op, pa, pb, n, out.ctypes.data_as(C.POINTER(C.c_uint64))), "mnt753_test_tower_op")
    return out.reshape(n, -1)


def test_miller_loop(curve, split, P, Q):
    """mnt753_test_miller_loop (test library): the unreduced Miller values [n, gt_words]"""
    p, pp = _u64(P)
    q, pq = _u64(Q)
    n = p.size // 24
    out = np.zeros((n, gt_words(curve)), dtype=np.uint64)
    _check(test_lib().mnt753_test_miller_loop(curve, split, pp, pq, n, out.ctypes.data_as(C.POINTER(C.c_uint64))), "mnt753_test_miller_loop")
    return out


def test_g2_endomorphism(curve, Q):
    """mnt753_test_g2_endomorphism (test library): psi(Q) of n twist points [n, affine_words] -> the same shape"""
    q, pq = _u64(Q)
    n = q.size // affine_words(curve, G2)
    out = np.zeros((n, affine_words(curve, G2)), dtype=np.uint64)
    _check(test_lib().mnt753_test_g2_endomorphism(curve, pq, n, out.ctypes.data_as(C.POINTER(C.c_uint64))), "mnt753_test_g2_endomorphism")
    return out


def test_g2_loop_multiple(curve, Q):
    """mnt753_test_g2_loop_multiple (test library): [t - 1] Q by the Miller loop's point steps, the identity as zero words"""
    q, pq = _u64(Q)
    n = q.size // affine_words(curve, G2)
    out = np.zeros((n, affine_words(curve, G2)), dtype=np.uint64)
    _check(test_lib().mnt753_test_g2_loop_multiple(curve, pq, n, out.ctypes.data_as(C.POINTER(C.c_uint64))), "mnt753_test_g2_loop_multiple")
    return out
