"""ctypes binding of include/g16_mi355x.h.  Loading fails loudly: the product has no fallback."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("G16_LIB", os.path.join(HERE, "libg16_mi355x.so"))  # G16_LIB: A/B-test another build

CURVE_ID = {"bls12_381": 0, "bn254": 1}
QAP_LIBSNARK, QAP_CIRCOM = 0, 1   # g16_qap
FQ_LIMBS = {"bls12_381": 6, "bn254": 4}

u64p = C.POINTER(C.c_uint64)
u32p = C.POINTER(C.c_uint32)


class G16Error(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(f"g16 status {status}: {msg}")
        self.status = status


class SynthesisError(G16Error):
    """mirrors ark_relations::r1cs::SynthesisError for the variants this path can produce"""


class PolynomialDegreeTooLarge(SynthesisError):
    pass


class UnexpectedIdentity(SynthesisError):
    """gamma or delta is zero (generator.rs:110-111)"""


class MalformedVerifyingKey(SynthesisError):
    """public inputs + 1 != gamma_abc_g1 (verifier.rs:29-31)"""


class Unsatisfiable(SynthesisError):
    """SynthesisError::Unsatisfiable: the assignment fails a constraint (status 12, g16_prove_checked).  `.row` is the first failing
    row (which_is_unsatisfied), `.n_unsatisfied` how many rows fail, `.a` / `.b` / `.c` the three sums of that row as Montgomery limbs
    (None when the status came without a g16_check_result)"""

    def __init__(self, status: int, msg: str, result: "Optional[CheckResultC]" = None):
        super().__init__(status, msg)
        self.row = int(result.first_row) if result is not None else None
        self.n_unsatisfied = int(result.n_unsatisfied) if result is not None else None
        self.a, self.b, self.c = (np.array(list(getattr(result, k)), dtype=np.uint64) if result is not None else None for k in "abc")


PK_BYTES_SECTIONS = ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2", "gamma_abc_g1", "beta_g1", "delta_g1", "a_query", "b_g1_query",
                     "b_g2_query", "h_query", "l_query")   # a serialized ProvingKey in file order (g16_pk_bytes_info)


class InvalidData(G16Error):
    """ark_serialize::SerializationError::InvalidData.  From g16_pk_load_bytes it names the first failing point of the key in file
    order: `.section` (a name of PK_BYTES_SECTIONS), `.index` within that section, `.reason` (0 the bytes do not decode, 2 off the
    curve, 3 outside the prime-order subgroup) and `.n_bad`, the failing points of the whole key; None from every other call"""

    def __init__(self, status: int, msg: str, info: "Optional[PkBytesInfoC]" = None):
        super().__init__(status, msg)
        named = info is not None and info.bad_section >= 0
        self.section = PK_BYTES_SECTIONS[info.bad_section] if named else None
        self.index = int(info.bad_index) if named else None
        self.reason = int(info.bad_reason) if named else None
        self.n_bad = int(info.n_bad) if named else None


class QueryC(C.Structure):
    _fields_ = [("points", C.c_void_p), ("count", C.c_uint64), ("start", C.c_uint64)]


class PkViewC(C.Structure):
    _fields_ = [
        ("alpha_g1", u64p), ("beta_g1", u64p), ("delta_g1", u64p), ("beta_g2", u64p), ("delta_g2", u64p),
        ("a_query0", u64p), ("b_g1_query0", u64p), ("b_g2_query0", u64p),
        ("a", QueryC), ("b_g1", QueryC), ("b_g2", QueryC), ("h", QueryC), ("l", QueryC),
        ("flags", C.c_uint32),
    ]


class CsrViewC(C.Structure):
    _fields_ = [("row_ptr", u64p), ("col", u32p), ("val", u64p)]


class ToxicWasteC(C.Structure):
    _fields_ = [(n, C.c_uint64 * 4) for n in ("alpha", "beta", "gamma", "delta", "t")]


class ParamsViewC(C.Structure):
    _fields_ = [(n, u64p) for n in ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "delta_g2", "gamma_g2", "gamma_abc_g1")] + \
               [(n, C.c_void_p) for n in ("a_query", "b_g1_query", "b_g2_query", "h_query", "l_query")] + [("flags", C.c_uint32)]


class SrsViewC(C.Structure):
    """g16_srs_view"""
    _fields_ = [("tau_g1", u64p), ("n_tau_g1", C.c_uint64), ("tau_g2", u64p), ("n_tau_g2", C.c_uint64), ("alpha_tau_g1", u64p),
                ("beta_tau_g1", u64p), ("n_alpha_beta", C.c_uint64), ("beta_g2", u64p)]


class SrsTimingsC(C.Structure):
    """g16_srs_timings"""
    _fields_ = [(n, C.c_double) for n in ("transforms_ms", "products_ms", "h_ms", "delta_ms")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class CeremonyInfoC(C.Structure):
    """g16_ceremony_info"""
    _fields_ = [("flags", C.c_uint32), ("bad_array", C.c_uint32), ("bad_index", C.c_uint64), ("bad_reason", C.c_uint32), ("reserved", C.c_uint32)]


class CeremonyTimingsC(C.Structure):
    """g16_ceremony_timings"""
    _fields_ = [(n, C.c_double) for n in ("upload_ms", "membership_ms", "sort_ms", "passes_ms", "reductions_ms", "pairings_ms")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class TauContributionC(C.Structure):
    """g16_tau_contribution"""
    _fields_ = [(n, u64p) for n in ("tau_g2", "alpha_g2", "beta_g2")]


class Phase1TimingsC(C.Structure):
    """g16_phase1_timings"""
    _fields_ = [(n, C.c_double) for n in ("upload_ms", "powers_ms", "mul_g1_ms", "mul_g2_ms", "download_ms")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class KeyFoldC(C.Structure):
    """g16_key_fold"""
    _fields_ = [(n, u64p) for n in ("a", "b_g1", "b_g2", "gamma_abc", "l", "h")]


class KeycheckTimingsC(C.Structure):
    """g16_keycheck_timings"""
    _fields_ = [(n, C.c_double) for n in ("upload_ms", "membership_ms", "rows_ms", "transforms_ms", "sorts_ms", "passes_ms", "reductions_ms",
                                          "pairings_ms", "window_bits", "windows")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class LagrangeSrsViewC(C.Structure):
    """g16_lagrange_srs_view"""
    _fields_ = [(n, u64p) for n in ("u_g1", "alpha_u_g1", "beta_u_g1", "u_g2", "h_g1", "tau_g1_0", "alpha_g1_0", "beta_g1_0", "tau_g2_0", "beta_g2")] + \
               [("log_n", C.c_int32), ("qap", C.c_int32)]


class LagrangeTimingsC(C.Structure):
    """g16_lagrange_timings"""
    _fields_ = [(n, C.c_double) for n in ("u_g1_ms", "alpha_u_g1_ms", "beta_u_g1_ms", "u_g2_ms", "h_ms", "products_ms")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class VkViewC(C.Structure):
    _fields_ = [(n, u64p) for n in ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2", "gamma_abc_g1")] + [("n_gamma_abc", C.c_uint64)]


class ProofC(C.Structure):
    _fields_ = [("a", C.c_uint64 * 12), ("b", C.c_uint64 * 24), ("c", C.c_uint64 * 12)]


class PartialC(C.Structure):
    _fields_ = [("h", C.c_uint64 * 24), ("l", C.c_uint64 * 24), ("a", C.c_uint64 * 24), ("b_g1", C.c_uint64 * 24),
                ("b_g2", C.c_uint64 * 48)]


class DiagC(C.Structure):
    _fields_ = [("mad_per_s", C.c_double), ("mads_per_add_g1", C.c_double), ("mads_per_add_g2", C.c_double),
                ("mads_per_product", C.c_double), ("limbs", C.c_int)]


class PkInfoC(C.Structure):
    _fields_ = [("window_bits_z", C.c_int), ("window_bits_h", C.c_int), ("table_fallback", C.c_int), ("bucket_shard_rank", C.c_int),
                ("bucket_shard_world", C.c_int), ("n_devices", C.c_int), ("device_bytes", C.c_uint64)]

    FALLBACK = {0: "window tables", 1: "plain bases by request (G16_MSM_PRECOMP=0)", 2: "plain bases: a query is too long for merged entries",
                3: "plain bases: the window tables did not fit in HBM (allocation failed or G16_PK_TABLE_BUDGET_MB)"}

    def as_dict(self):
        d = {n: int(getattr(self, n)) for n, _ in self._fields_}
        d["held_as"] = self.FALLBACK.get(int(self.table_fallback), "?")
        return d


class CheckResultC(C.Structure):
    """g16_check_result"""
    _fields_ = [("n_unsatisfied", C.c_uint64), ("first_row", C.c_uint64), ("a", C.c_uint64 * 4), ("b", C.c_uint64 * 4), ("c", C.c_uint64 * 4)]


class PkBytesInfoC(C.Structure):
    """g16_pk_bytes_info"""
    _fields_ = [("consumed", C.c_uint64), ("count", C.c_uint64 * 12), ("bad_section", C.c_int32), ("bad_reason", C.c_int32),
                ("bad_index", C.c_uint64), ("n_bad", C.c_uint64)]

    def counts(self) -> dict:
        return {name: int(self.count[k]) for k, name in enumerate(PK_BYTES_SECTIONS)}


class PassLabJobC(C.Structure):
    """g16_pass_lab_job"""
    _fields_ = [("table", u64p), ("base_count", C.c_uint64), ("shift", C.c_int64), ("counts", u32p), ("sorted", u32p), ("n_sorted", C.c_uint64),
                ("record_cap", C.c_uint64), ("records", u32p), ("n_records", C.c_uint64), ("offsets", u32p), ("task_off", u32p), ("heavy", u32p),
                ("out_affine", u64p)]


class SortLabInfoC(C.Structure):
    """g16_sort_lab_info"""
    _fields_ = [("c", C.c_int32), ("W", C.c_int32), ("groups", C.c_int32), ("merged", C.c_int32), ("B", C.c_uint32), ("Lmax", C.c_uint32),
                ("max_tasks", C.c_uint32), ("max_segments", C.c_uint32), ("K", C.c_uint32 * 10), ("n_sorted", C.c_uint32), ("reserved", C.c_uint32)]


class TimingsC(C.Structure):
    _fields_ = [(n, C.c_double) for n in (
        "witness_map_ms", "msm_h_ms", "msm_l_ms", "msm_a_ms", "msm_b_g1_ms", "msm_b_g2_ms", "scalar_prep_ms", "finish_ms",
        "total_ms", "bucket_pass_ms")] + [("bucket_ms", C.c_double * 5), ("window_bits", C.c_double), ("windows", C.c_double), ("ntt_ms", C.c_double),
                                  ("g1_pass_launches", C.c_double)]

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_ if n != "bucket_ms"}
        d["bucket_ms"] = list(self.bucket_ms)
        return d


EXPORTS = [
    "g16_ctx_create", "g16_ctx_create_multi", "g16_ctx_num_devices", "g16_ctx_peer_access", "g16_ctx_destroy", "g16_ctx_stream", "g16_pk_load", "g16_pk_free", "g16_circuit_load", "g16_circuit_free",
    "g16_circuit_domain_size", "g16_prove", "g16_prove_partial", "g16_prove_finalize", "g16_finalize_host", "g16_prove_partial_h", "g16_dwm_create",
    "g16_dwm_free", "g16_dwm_local_size", "g16_dwm_stage", "g16_dwm_stage_async", "g16_ctx_wm_stream", "g16_prove_partial_prepare", "g16_prove_finalize_prepare", "g16_get_timings", "g16_diag_valu", "g16_witness_map",
    "g16_msm_g1", "g16_msm_g2", "g16_ntt", "g16_synth_bases", "g16_synth_circuit", "g16_host_field_op", "g16_host_group_op",
    "g16_host_msm_model", "g16_host_selftest", "g16_strerror", "g16_last_error", "g16_version", "g16_generate_parameters",
    "g16_host_qap_evaluations", "g16_serialized_point_size", "g16_serialize_points", "g16_deserialize_points",
    "g16_pk_load_bucket_shard", "g16_pk_rebind_bucket_shard", "g16_pk_get_info", "g16_msm_bucket_shard", "g16_host_msm_model_shard",
    "g16_abi_version", "g16_struct_size", "g16_get_timings_sized", "g16_pk_get_info_sized",
    "g16_pvk_load", "g16_pvk_free", "g16_pvk_alpha_beta", "g16_verify_batch", "g16_verify_batch_prepared", "g16_pairing",
    "g16_host_pairing", "g16_host_verify", "g16_verify_aggregate", "g16_host_verify_aggregate", "g16_host_verify_aggregate_gt",
    "g16_dev_fp30_op", "g16_host_fp30_op", "g16_dev_msm_reduce_lab", "g16_dev_msm_reduce_batch_lab", "g16_dev_window_table_lab", "g16_dev_pairing_op", "g16_host_pairing_op",
    "g16_dev_std_op", "g16_host_std_op",
    "g16_dev_msm_pass_lab", "g16_dev_msm_sort_lab", "g16_dev_msm_parts_lab", "g16_host_msm_parts_lab",
    "g16_dev_pvk_tables", "g16_dev_prepare_inputs", "g16_host_pvk_tables", "g16_host_prepare_inputs",
    "g16_check_subgroups", "g16_check_proof_subgroups", "g16_verify_aggregate_checked", "g16_host_check_subgroups",
    "g16_decompress_points", "g16_decompress_proofs", "g16_host_decompress_points", "g16_verify_aggregate_bytes",
    "g16_verify_aggregate_mixed", "g16_host_verify_aggregate_mixed", "g16_host_verify_aggregate_mixed_gt",
    "g16_circuit_load_qap", "g16_circuit_qap", "g16_generate_parameters_qap", "g16_h_query_len", "g16_host_h_query_scalars",
    "g16_circuit_attach_c", "g16_circuit_check", "g16_prove_checked", "g16_host_circuit_check",
    "g16_decode_points", "g16_host_decode_points", "g16_host_pk_bytes_layout", "g16_pk_load_bytes", "g16_pk_load_bytes_timings",
    "g16_srs_segment_len", "g16_generate_parameters_srs", "g16_params_apply_delta", "g16_group_ntt", "g16_srs_from_trapdoor",
    "g16_srs_get_timings", "g16_host_group_ntt", "g16_host_generate_parameters_srs",
]
# libg16_ceremony.so, the companion library of the ceremony checks (include/g16_ceremony.h)
CEREMONY_EXPORTS = [
    "g16_rlc_sums", "g16_rlc_plan", "g16_srs_check", "g16_params_check_delta", "g16_ceremony_get_timings", "g16_host_rlc_sums", "g16_host_srs_check",
    "g16_host_params_check_delta",
]
# libg16_phase1.so, the companion library of phase 1 (include/g16_phase1.h)
PHASE1_EXPORTS = [
    "g16_batch_scalar_mul", "g16_host_batch_scalar_mul", "g16_host_batch_scalar_mul_windowed", "g16_srs_contribute", "g16_host_srs_contribute",
    "g16_phase1_get_timings", "g16_srs_check_contribution", "g16_host_srs_check_contribution",
]
# libg16_keycheck.so, the companion library of the key check without the derivation (include/g16_keycheck.h)
KEYCHECK_EXPORTS = [
    "g16_params_check_derivation", "g16_key_fold_from_srs", "g16_keycheck_get_timings", "g16_host_params_check_derivation",
    "g16_host_key_fold_from_srs",
]
# libg16_lagrange.so, the companion library of the Lagrange form of an SRS and the key from it (include/g16_lagrange.h)
LAGRANGE_EXPORTS = [
    "g16_group_ntt_windowed", "g16_host_group_ntt_windowed", "g16_srs_lagrange", "g16_host_srs_lagrange", "g16_generate_parameters_lagrange",
    "g16_host_generate_parameters_lagrange", "g16_lagrange_get_timings",
]


def ptr64(a: Optional[np.ndarray]):
    if a is None:
        return None
    assert a.dtype == np.uint64 and a.flags["C_CONTIGUOUS"], "expected a C-contiguous uint64 array"
    return a.ctypes.data_as(u64p)


def ptr32(a: np.ndarray):
    assert a.dtype == np.uint32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(u32p)


def _ceremony_argtypes(c):
    c.g16_rlc_sums.argtypes = [C.c_void_p, C.c_int, u64p, C.c_uint64, u64p, u64p, u64p]
    c.g16_rlc_plan.argtypes = [C.c_uint64, u32p]
    c.g16_host_rlc_sums.argtypes = [C.c_int, C.c_int, u64p, C.c_uint64, u64p, u64p, u64p]
    c.g16_srs_check.argtypes = [C.c_void_p, C.POINTER(SrsViewC), u64p, C.c_uint64, C.POINTER(CeremonyInfoC)]
    c.g16_host_srs_check.argtypes = [C.c_int] + c.g16_srs_check.argtypes[1:]
    c.g16_params_check_delta.argtypes = [C.c_void_p, C.POINTER(ParamsViewC), C.POINTER(ParamsViewC), C.c_uint64, C.c_uint64, C.c_uint64,
                                         C.c_uint64, u64p, C.c_uint64, C.POINTER(CeremonyInfoC)]
    c.g16_host_params_check_delta.argtypes = [C.c_int] + c.g16_params_check_delta.argtypes[1:]
    c.g16_ceremony_get_timings.argtypes = [C.c_void_p, C.POINTER(CeremonyTimingsC)]


def _phase1_argtypes(c):
    c.g16_batch_scalar_mul.argtypes = [C.c_void_p, C.c_int, u64p, u64p, C.c_uint64, u64p]
    c.g16_host_batch_scalar_mul.argtypes = [C.c_int, C.c_int, u64p, u64p, C.c_uint64, u64p]
    c.g16_host_batch_scalar_mul_windowed.argtypes = c.g16_host_batch_scalar_mul.argtypes
    c.g16_srs_contribute.argtypes = [C.c_void_p, u64p, u64p, u64p, C.POINTER(SrsViewC), C.POINTER(TauContributionC), C.POINTER(Phase1TimingsC)]
    c.g16_host_srs_contribute.argtypes = [C.c_int] + c.g16_srs_contribute.argtypes[1:]
    c.g16_phase1_get_timings.argtypes = [C.c_void_p, C.POINTER(Phase1TimingsC)]
    c.g16_srs_check_contribution.argtypes = [C.c_void_p, C.POINTER(SrsViewC), C.POINTER(SrsViewC), C.POINTER(TauContributionC), u64p, C.c_uint64,
                                             C.POINTER(CeremonyInfoC)]
    c.g16_host_srs_check_contribution.argtypes = [C.c_int] + c.g16_srs_check_contribution.argtypes[1:]


def _keycheck_argtypes(c):
    shape = [C.POINTER(CsrViewC), C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(SrsViewC)]
    c.g16_params_check_derivation.argtypes = [C.c_void_p] + shape + [C.POINTER(ParamsViewC), u64p, C.c_uint64, C.POINTER(CeremonyInfoC)]
    c.g16_host_params_check_derivation.argtypes = [C.c_int] + c.g16_params_check_derivation.argtypes[1:]
    c.g16_key_fold_from_srs.argtypes = [C.c_void_p] + shape + [u64p, C.c_uint64, C.POINTER(KeyFoldC)]
    c.g16_host_key_fold_from_srs.argtypes = [C.c_int] + c.g16_key_fold_from_srs.argtypes[1:]
    c.g16_keycheck_get_timings.argtypes = [C.c_void_p, C.POINTER(KeycheckTimingsC)]


def _lagrange_argtypes(c):
    c.g16_group_ntt_windowed.argtypes = [C.c_void_p, C.c_int, u64p, C.c_int, C.c_int, u64p]
    c.g16_host_group_ntt_windowed.argtypes = [C.c_int, C.c_int, u64p, C.c_int, C.c_int, u64p]
    c.g16_srs_lagrange.argtypes = [C.c_void_p, C.POINTER(SrsViewC), C.c_int, C.c_int, C.POINTER(LagrangeSrsViewC)]
    c.g16_host_srs_lagrange.argtypes = [C.c_int] + c.g16_srs_lagrange.argtypes[1:]
    c.g16_generate_parameters_lagrange.argtypes = [C.c_void_p, C.POINTER(CsrViewC), C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(LagrangeSrsViewC),
                                                   C.POINTER(ParamsViewC)]
    c.g16_host_generate_parameters_lagrange.argtypes = [C.c_int] + c.g16_generate_parameters_lagrange.argtypes[1:]
    c.g16_lagrange_get_timings.argtypes = [C.c_void_p, C.POINTER(LagrangeTimingsC)]


class Lib:
    def __init__(self, path: str = LIB_PATH):
        if not os.path.exists(path):
            raise ImportError(
                f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  groth16_amd has no CPU fallback.")
        self.path = path
        self._companions = {}   # file name -> the loaded companion library (cer, ph1, kc, lag)
        # One HIP runtime per process: torch wheels bundle their own libamdhip64, and this library links the system one.  Whichever is
        # loaded first serves both (same soname); loaded in the order library -> torch, g16_ctx_create found no device on the GPU box
        # (round 3: `python __graft_entry__.py smoke`, where build() loads the library before smoke() imports torch).  So when torch is
        # installed it goes first -- every Python user of this package needs it for device buffers anyway; a C / Rust caller has no torch
        # in the process and is not affected.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        self.c = C.CDLL(path)
        c = self.c
        c.g16_strerror.restype = C.c_char_p
        c.g16_last_error.restype = C.c_char_p
        c.g16_version.restype = C.c_char_p
        c.g16_ctx_stream.restype = C.c_void_p
        c.g16_ctx_stream.argtypes = [C.c_void_p]
        c.g16_ctx_wm_stream.restype = C.c_void_p
        c.g16_ctx_wm_stream.argtypes = [C.c_void_p]
        c.g16_dwm_stage_async.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                          C.c_void_p]
        c.g16_circuit_domain_size.restype = C.c_uint64
        c.g16_circuit_domain_size.argtypes = [C.c_void_p]
        c.g16_ctx_create.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        c.g16_ctx_create_multi.argtypes = [C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p)]
        c.g16_ctx_num_devices.argtypes = [C.c_void_p]
        c.g16_ctx_peer_access.argtypes = [C.c_void_p, C.c_int, C.c_int]
        c.g16_ctx_destroy.argtypes = [C.c_void_p]
        c.g16_ctx_destroy.restype = None
        c.g16_pk_load.argtypes = [C.c_void_p, C.POINTER(PkViewC), C.POINTER(C.c_void_p)]
        c.g16_pk_free.argtypes = [C.c_void_p]
        c.g16_pk_free.restype = None
        c.g16_pk_load_bucket_shard.argtypes = [C.c_void_p, C.POINTER(PkViewC), C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        c.g16_pk_rebind_bucket_shard.argtypes = [C.c_void_p, C.c_int, C.c_int]
        c.g16_pk_get_info.argtypes = [C.c_void_p, C.POINTER(PkInfoC)]
        c.g16_msm_bucket_shard.argtypes = [C.c_void_p, C.c_int, u64p, u64p, C.c_uint64, C.c_int, C.c_int, u64p]
        c.g16_host_msm_model_shard.argtypes = [C.c_int, C.c_int, u64p, u64p, C.c_uint64, C.c_int, C.c_int, C.c_int, u64p]
        c.g16_circuit_load.argtypes = [C.c_void_p, C.POINTER(CsrViewC), C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_void_p)]
        c.g16_circuit_load_qap.argtypes = [C.c_void_p, C.POINTER(CsrViewC), C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(C.c_void_p)]
        c.g16_circuit_qap.argtypes = [C.c_void_p]
        c.g16_circuit_free.argtypes = [C.c_void_p]
        c.g16_circuit_free.restype = None
        c.g16_prove.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, u64p, u64p, C.POINTER(ProofC)]
        c.g16_prove_partial.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int,
                                        C.POINTER(PartialC)]
        c.g16_prove_partial_h.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.c_int,
                                          C.POINTER(PartialC)]
        c.g16_prove_partial_prepare.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
        c.g16_prove_finalize_prepare.argtypes = [C.c_void_p, C.c_void_p, u64p, u64p]
        c.g16_dwm_create.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        c.g16_dwm_free.argtypes = [C.c_void_p]
        c.g16_dwm_free.restype = None
        c.g16_dwm_local_size.argtypes = [C.c_void_p]
        c.g16_dwm_local_size.restype = C.c_uint64
        c.g16_dwm_stage.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                    C.c_void_p]
        c.g16_prove_finalize.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(PartialC), C.c_int, u64p, u64p, C.POINTER(ProofC)]
        c.g16_finalize_host.argtypes = [C.c_int, C.POINTER(PkViewC), C.POINTER(PartialC), C.c_int, u64p, u64p, C.POINTER(ProofC)]
        c.g16_get_timings.argtypes = [C.c_void_p, C.POINTER(TimingsC)]
        c.g16_struct_size.argtypes = [C.c_int]
        c.g16_struct_size.restype = C.c_uint64
        c.g16_get_timings_sized.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        c.g16_pk_get_info_sized.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        c.g16_diag_valu.argtypes = [C.c_void_p, C.POINTER(DiagC)]
        c.g16_witness_map.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, u64p]
        c.g16_msm_g1.argtypes = [C.c_void_p, u64p, u64p, C.c_uint64, u64p]
        c.g16_msm_g2.argtypes = [C.c_void_p, u64p, u64p, C.c_uint64, u64p]
        c.g16_ntt.argtypes = [C.c_void_p, u64p, C.c_int, C.c_int, C.c_int]
        c.g16_synth_bases.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]
        c.g16_synth_circuit.argtypes = [C.c_int, C.c_int, C.c_uint64, u64p, u64p, u32p, u32p, u32p, u64p]
        c.g16_host_field_op.argtypes = [C.c_int, C.c_int, C.c_int, u64p, u64p, u64p]
        c.g16_host_group_op.argtypes = [C.c_int, C.c_int, C.c_int, u64p, u64p, u64p]
        c.g16_host_selftest.argtypes = [C.c_int, C.c_uint64, C.c_int]
        c.g16_host_msm_model.argtypes = [C.c_int, C.c_int, u64p, u64p, C.c_uint64, C.c_int, u64p]
        c.g16_generate_parameters.argtypes = [C.c_void_p, C.POINTER(CsrViewC), C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(ToxicWasteC),
                                              u64p, u64p, C.POINTER(ParamsViewC)]
        c.g16_generate_parameters_qap.argtypes = [C.c_void_p, C.POINTER(CsrViewC), C.c_uint64, C.c_uint64, C.c_uint64, C.c_int,
                                                  C.POINTER(ToxicWasteC), u64p, u64p, C.POINTER(ParamsViewC)]
        c.g16_h_query_len.argtypes = [C.c_int, C.c_uint64]
        c.g16_h_query_len.restype = C.c_uint64
        c.g16_host_h_query_scalars.argtypes = [C.c_int, C.c_int, C.c_uint64, u64p, u64p, u64p]
        c.g16_serialized_point_size.restype = C.c_uint64
        c.g16_serialized_point_size.argtypes = [C.c_int, C.c_int, C.c_int]
        c.g16_serialize_points.argtypes = [C.c_int, C.c_int, C.c_int, u64p, C.c_uint64, C.c_char_p]
        c.g16_deserialize_points.argtypes = [C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_uint64, C.c_int, u64p]
        c.g16_host_qap_evaluations.argtypes = [C.c_int, C.POINTER(CsrViewC), C.c_uint64, C.c_uint64, C.c_uint64, u64p, u64p, u64p, u64p, u64p]

        c.g16_pvk_load.argtypes = [C.c_void_p, C.POINTER(VkViewC), C.POINTER(C.c_void_p)]
        c.g16_pvk_free.argtypes = [C.c_void_p]
        c.g16_pvk_free.restype = None
        c.g16_pvk_alpha_beta.argtypes = [C.c_void_p, u64p]
        c.g16_verify_batch.argtypes = [C.c_void_p, C.c_void_p, u64p, C.c_uint64, u64p, C.c_uint64, C.c_void_p]
        c.g16_verify_batch_prepared.argtypes = [C.c_void_p, C.c_void_p, u64p, u64p, C.c_uint64, C.c_void_p]
        c.g16_pairing.argtypes = [C.c_void_p, u64p, u64p, C.c_uint64, u64p]
        c.g16_host_pairing.argtypes = [C.c_int, u64p, u64p, C.c_uint64, u64p]
        c.g16_host_verify.argtypes = [C.c_int, C.POINTER(VkViewC), u64p, u64p, C.c_uint64, C.c_void_p]
        c.g16_verify_aggregate.argtypes = [C.c_void_p, C.c_void_p, u64p, C.c_uint64, u64p, C.c_uint64, u64p, C.c_void_p]
        c.g16_host_verify_aggregate.argtypes = [C.c_int, C.POINTER(VkViewC), u64p, C.c_uint64, u64p, C.c_uint64, u64p, C.c_void_p]
        c.g16_host_verify_aggregate_gt.argtypes = [C.c_int, C.POINTER(VkViewC), u64p, C.c_uint64, u64p, C.c_uint64, u64p, u64p, u64p]
        c.g16_verify_aggregate_checked.argtypes = c.g16_verify_aggregate.argtypes
        c.g16_check_subgroups.argtypes = [C.c_void_p, C.c_int, u64p, C.c_uint64, C.c_void_p]
        c.g16_check_proof_subgroups.argtypes = [C.c_void_p, u64p, C.c_uint64, C.c_void_p]
        c.g16_host_check_subgroups.argtypes = [C.c_int, C.c_int, u64p, C.c_uint64, C.c_void_p]
        c.g16_decompress_points.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, u64p, C.c_void_p]
        c.g16_decompress_proofs.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, u64p, C.c_void_p]
        c.g16_host_decompress_points.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_uint64, u64p, C.c_void_p]
        c.g16_verify_aggregate_bytes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, u64p, C.c_uint64, u64p, C.c_void_p]
        c.g16_verify_aggregate_mixed.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_uint64, u32p, u64p, C.c_uint64, u64p, C.c_uint64, u64p,
                                                 C.c_int, C.c_void_p]
        c.g16_host_verify_aggregate_mixed.argtypes = [C.c_int, C.POINTER(VkViewC), C.c_uint64, u32p, u64p, C.c_uint64, u64p, C.c_uint64, u64p,
                                                      C.c_void_p]
        c.g16_host_verify_aggregate_mixed_gt.argtypes = [C.c_int, C.POINTER(VkViewC), C.c_uint64, u32p, u64p, C.c_uint64, u64p, C.c_uint64, u64p,
                                                         u64p, u64p]
        c.g16_circuit_attach_c.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(CsrViewC)]
        c.g16_circuit_check.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.POINTER(CheckResultC)]
        c.g16_prove_checked.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, u64p, u64p, C.POINTER(ProofC),
                                        C.POINTER(CheckResultC)]
        c.g16_host_circuit_check.argtypes = [C.c_int, C.POINTER(CsrViewC), C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(CheckResultC)]
        c.g16_decode_points.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_uint64, u64p, C.c_void_p]
        c.g16_host_decode_points.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_uint64, u64p, C.c_void_p]
        c.g16_host_pk_bytes_layout.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64]
        c.g16_pk_load_bytes.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_void_p, C.c_uint64]
        c.g16_pk_load_bytes_timings.argtypes = [C.POINTER(C.c_double), C.c_int]
        c.g16_srs_segment_len.argtypes = []
        c.g16_srs_segment_len.restype = C.c_uint64
        c.g16_generate_parameters_srs.argtypes = [C.c_void_p, C.POINTER(CsrViewC), C.c_uint64, C.c_uint64, C.c_uint64, C.c_int,
                                                  C.POINTER(SrsViewC), C.POINTER(ParamsViewC)]
        c.g16_host_generate_parameters_srs.argtypes = [C.c_int] + c.g16_generate_parameters_srs.argtypes[1:]
        c.g16_params_apply_delta.argtypes = [C.c_void_p, u64p, C.POINTER(ParamsViewC), C.c_uint64, C.c_uint64]
        c.g16_group_ntt.argtypes = [C.c_void_p, C.c_int, u64p, C.c_int, C.c_int, u64p]
        c.g16_host_group_ntt.argtypes = [C.c_int, C.c_int, u64p, C.c_int, C.c_int, u64p]
        c.g16_srs_from_trapdoor.argtypes = [C.c_void_p, u64p, u64p, u64p, u64p, u64p, C.c_uint64, C.c_uint64, C.POINTER(SrsViewC)]
        c.g16_srs_get_timings.argtypes = [C.c_void_p, C.POINTER(SrsTimingsC)]
        c.g16_dev_fp30_op.argtypes = [C.c_void_p, C.c_int, C.c_int, u32p, C.c_uint64, u32p]
        c.g16_host_fp30_op.argtypes = [C.c_int, C.c_int, C.c_int, u32p, C.c_uint64, u32p]
        c.g16_dev_pairing_op.argtypes = [C.c_void_p, C.c_int, u32p, C.c_uint64, u32p]
        c.g16_host_pairing_op.argtypes = [C.c_int, C.c_int, u32p, C.c_uint64, u32p]
        c.g16_dev_std_op.argtypes = [C.c_void_p, C.c_int, C.c_int, u32p, C.c_uint64, u32p]
        c.g16_host_std_op.argtypes = [C.c_int, C.c_int, C.c_int, u32p, C.c_uint64, u32p]
        c.g16_dev_msm_reduce_lab.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, u32p, u32p, C.c_uint64, u32p, u64p]
        c.g16_dev_msm_reduce_batch_lab.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.POINTER(u32p),
                                                   C.POINTER(u32p), u64p, C.POINTER(u32p), C.POINTER(u64p)]
        c.g16_dev_window_table_lab.argtypes = [C.c_void_p, C.c_int, u64p, C.c_uint64, C.c_int, C.c_int, u64p]
        c.g16_dev_msm_pass_lab.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(PassLabJobC),
                                           C.c_int]
        c.g16_dev_msm_parts_lab.argtypes = c.g16_dev_msm_pass_lab.argtypes
        c.g16_host_msm_parts_lab.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(PassLabJobC)]
        c.g16_dev_msm_sort_lab.argtypes = [C.c_void_p, u64p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.POINTER(SortLabInfoC), u32p, u32p, u32p,
                                           C.c_uint64, u32p, C.c_uint64]
        c.g16_dev_pvk_tables.argtypes = [C.c_void_p, C.c_void_p, C.c_int, u64p]
        c.g16_dev_prepare_inputs.argtypes = [C.c_void_p, C.c_void_p, u64p, C.c_uint64, C.c_uint64, u64p]
        c.g16_host_pvk_tables.argtypes = [C.c_int, C.POINTER(VkViewC), u64p]
        c.g16_host_prepare_inputs.argtypes = [C.c_int, C.POINTER(VkViewC), u64p, C.c_uint64, C.c_uint64, u64p]

    def _companion(self, name: str, set_argtypes):
        """a companion library beside the library, loaded on first use and kept; set_argtypes(c) declares its entry points"""
        if name not in self._companions:
            path = os.path.join(os.path.dirname(self.path), name)
            if not os.path.exists(path):
                raise ImportError(f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
            c = C.CDLL(path)
            set_argtypes(c)
            self._companions[name] = c
        return self._companions[name]

    @property
    def cer(self):
        """libg16_ceremony.so (it links against the library and shares its contexts)"""
        return self._companion("libg16_ceremony.so", _ceremony_argtypes)

    @property
    def ph1(self):
        """libg16_phase1.so (it links against the library and the ceremony library)"""
        return self._companion("libg16_phase1.so", _phase1_argtypes)

    @property
    def kc(self):
        """libg16_keycheck.so (it links against the library and its two other companions)"""
        return self._companion("libg16_keycheck.so", _keycheck_argtypes)

    @property
    def lag(self):
        """libg16_lagrange.so (it links against the library and its three other companions)"""
        return self._companion("libg16_lagrange.so", _lagrange_argtypes)

    def check(self, status: int, check_result: "Optional[CheckResultC]" = None, pk_bytes_info: "Optional[PkBytesInfoC]" = None):
        """check_result: the g16_check_result a checked call filled, carried by Unsatisfiable; pk_bytes_info: the g16_pk_bytes_info
        g16_pk_load_bytes filled, carried by InvalidData"""
        if status == 0:
            return
        msg = self.c.g16_strerror(status).decode()
        detail = self.c.g16_last_error().decode()
        if detail:
            msg += " | " + detail
        if status == 1:
            raise PolynomialDegreeTooLarge(status, msg)
        if status == 8:
            raise UnexpectedIdentity(status, msg)
        if status == 9:
            raise InvalidData(status, msg, pk_bytes_info)
        if status == 11:
            raise MalformedVerifyingKey(status, msg)
        if status == 12:
            raise Unsatisfiable(status, msg, check_result)
        raise G16Error(status, msg)

    def version(self) -> str:
        return self.c.g16_version().decode()


def msm_reduce_lab(lb: "Lib", ctx, g2: bool, merged: bool, c: int, groups: int, G: int, nparts: np.ndarray, records: np.ndarray,
                   affine_words: int):
    """g16_dev_msm_reduce_lab (test hook): the prover's MSM reductions and host fold on caller-made partial sums.
    nparts: uint32 [groups * 2^(c-1)] partial sums per bucket; records: uint32 [sum(nparts), record words] raw lazy limbs.
    Returns (every bucket's first slot after the combine stages, uint32 [buckets, record words]; the folded affine point,
    uint64 [affine_words])."""
    nparts = np.ascontiguousarray(nparts, dtype=np.uint32)
    records = np.ascontiguousarray(records, dtype=np.uint32)
    assert nparts.shape == (groups << (c - 1),) and records.ndim == 2 and records.shape[0] == int(nparts.sum())
    first = np.full((nparts.shape[0], records.shape[1]), 0xDEADBEEF, dtype=np.uint32)
    out = np.zeros(affine_words, dtype=np.uint64)
    lb.check(lb.c.g16_dev_msm_reduce_lab(ctx, int(g2), int(merged), c, groups, G, ptr32(nparts), ptr32(records), records.shape[0],
                                         ptr32(first), ptr64(out)))
    return first, out


def msm_reduce_batch_lab(lb: "Lib", ctx, merged: bool, c: int, groups: int, G: int, jobs, early=None, affine_words: int = 0):
    """g16_dev_msm_reduce_batch_lab (test hook, G1): the reductions of up to four jobs over one plan as the launches a proof makes.
    jobs: a list of (nparts, records) as msm_reduce_lab takes them.  early=None: all jobs through msm_reduce_batch together; early=a
    set of job indices: those through msm_heavy_reduce_batch in one launch, the others through msm_heavy_reduce alone, then
    msm_reduce_batch with heavy_done.  Returns (status, results); results is None unless status == 0, else per job (first slots,
    folded affine point) as msm_reduce_lab returns them.  Nothing is checked here: refusing is the library's to do."""
    n = len(jobs)
    keep, outs = [], []
    np_arr, rec_arr, first_arr, out_arr = (u32p * max(n, 1))(), (u32p * max(n, 1))(), (u32p * max(n, 1))(), (u64p * max(n, 1))()
    n_rec = np.zeros(max(n, 1), dtype=np.uint64)
    for k, (nparts, records) in enumerate(jobs):
        nparts = np.ascontiguousarray(nparts, dtype=np.uint32)
        records = np.ascontiguousarray(records, dtype=np.uint32)
        assert records.ndim == 2
        first = np.full((nparts.shape[0], records.shape[1]), 0xDEADBEEF, dtype=np.uint32)
        out = np.zeros(affine_words, dtype=np.uint64)
        keep.append((nparts, records))
        outs.append((first, out))
        np_arr[k], rec_arr[k], first_arr[k], out_arr[k] = ptr32(nparts), ptr32(records.reshape(-1)), ptr32(first.reshape(-1)), ptr64(out)
        n_rec[k] = records.shape[0]
    mask = 0
    for j in (early or ()):
        mask |= 1 << j
    status = lb.c.g16_dev_msm_reduce_batch_lab(ctx, int(merged), c, groups, G, n, 0 if early is None else 1, mask, np_arr, rec_arr, ptr64(n_rec),
                                               first_arr, out_arr)
    return status, (outs if status == 0 else None)


PASS_LAB_GUARDS = 8


def msm_pass_lab(lb: "Lib", ctx, g2: bool, merged: bool, c: int, groups: int, G: int, lseg: int, rows: int, jobs, record_words: int,
                 affine_words: int, walk: str = "segment"):
    """g16_dev_msm_pass_lab (test hook): the bucket pass's walk on caller-made sorted lists, all jobs in one launch.
    jobs: a list of dicts with table (uint64 [rows * base_count, affine words]), base_count, shift, counts (uint32 [M]) and sorted
    (uint32 [S]).  Returns (status, results); results is None unless status == 0, else per job a dict: records (uint32
    [task_off[M] + 8, record words], the last 8 the guards), offsets, task_off, heavy (uint32 [M + 1] each) and out (uint64
    [affine_words], the folded sum).  Nothing is checked here: refusing is the library's to do."""
    M = groups << (c - 1)
    arr = (PassLabJobC * max(len(jobs), 1))()
    keep, outs = [], []
    for k, job in enumerate(jobs):
        table = np.ascontiguousarray(job["table"], dtype=np.uint64)
        counts = np.ascontiguousarray(job["counts"], dtype=np.uint32)
        srt = np.ascontiguousarray(job["sorted"], dtype=np.uint32)
        cap = job.get("record_cap", (len(srt) + max(lseg, 1) - 1) // max(lseg, 1) + M + PASS_LAB_GUARDS)
        o = {"records": np.zeros((max(cap, 1), record_words), dtype=np.uint32), "offsets": np.zeros(M + 1, dtype=np.uint32),
             "task_off": np.zeros(M + 1, dtype=np.uint32), "heavy": np.zeros(M + 1, dtype=np.uint32), "out": np.zeros(affine_words, dtype=np.uint64)}
        keep.append((table, counts, srt))
        outs.append(o)
        j = arr[k]
        j.table, j.base_count, j.shift = ptr64(table.reshape(-1)), int(job["base_count"]), int(job["shift"])
        j.counts, j.sorted, j.n_sorted, j.record_cap = ptr32(counts), ptr32(srt), int(job.get("n_sorted", len(srt))), cap
        j.records, j.offsets, j.task_off, j.heavy, j.out_affine = (ptr32(o["records"].reshape(-1)), ptr32(o["offsets"]), ptr32(o["task_off"]),
                                                                   ptr32(o["heavy"]), ptr64(o["out"]))
    if walk == "host":
        assert len(jobs) == 1 and not g2
        status = lb.c.g16_host_msm_parts_lab(ctx, int(merged), c, groups, lseg, rows, arr)
    else:
        entry = lb.c.g16_dev_msm_parts_lab if walk == "parts" else lb.c.g16_dev_msm_pass_lab
        status = entry(ctx, int(g2), int(merged), c, groups, G, lseg, rows, arr, len(jobs))
    if status != 0:
        return status, None
    for k, o in enumerate(outs):
        o["records"] = o["records"][:arr[k].n_records + (0 if walk == "host" else PASS_LAB_GUARDS)]
    return status, outs


def msm_parts_lab(lb: "Lib", ctx, g2: bool, merged: bool, c: int, groups: int, G: int, lmax: int, rows: int, jobs, record_words: int,
                  affine_words: int):
    """g16_dev_msm_parts_lab (test hook): msm_pass_lab with the bucket-part walk, lmax the longest part"""
    return msm_pass_lab(lb, ctx, g2, merged, c, groups, G, lmax, rows, jobs, record_words, affine_words, walk="parts")


def host_msm_parts_lab(lb: "Lib", curve_id: int, merged: bool, c: int, groups: int, lmax: int, rows: int, job, record_words: int,
                       affine_words: int):
    """g16_host_msm_parts_lab (host twin, G1): one job through the layout rule and the per-task walk compiled for the host.
    Returns (status, result) as msm_pass_lab does for one job; the records carry no guards."""
    status, outs = msm_pass_lab(lb, curve_id, False, merged, c, groups, 8, lmax, rows, [job], record_words, affine_words, walk="host")
    return status, (outs[0] if outs else None)


def msm_sort_lab(lb: "Lib", ctx, scalars: np.ndarray, merged_c: int = 0, shard_n: int = 1, shard_r: int = 0):
    """g16_dev_msm_sort_lab (test hook): sort_scalars on caller-made scalars (uint64 [n, 4], Montgomery limbs).
    Returns (status, result); result is None unless status == 0, else a dict: the g16_sort_lab_info fields, M, offsets, task_off,
    heavy (uint32 [M + 1] each) and sorted (uint32 [offsets[M]])."""
    scalars = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
    n = scalars.shape[0]
    bucket_cap = (1 << 20) + 1                  # 2^19 buckets at the largest plans (merged c = 20; per-window c = 16 has 17 x 2^15)
    sorted_cap = max(n, 1) * 128                # W <= 86 windows (c = 3)
    info = SortLabInfoC()
    offsets, task_off, heavy = (np.zeros(bucket_cap, dtype=np.uint32) for _ in range(3))
    srt = np.zeros(sorted_cap, dtype=np.uint32)
    status = lb.c.g16_dev_msm_sort_lab(ctx, ptr64(scalars.reshape(-1)), n, merged_c, shard_n, shard_r, C.byref(info), ptr32(offsets),
                                       ptr32(task_off), ptr32(heavy), bucket_cap, ptr32(srt), sorted_cap)
    if status != 0:
        return status, None
    M = info.groups * info.B
    res = {k: getattr(info, k) for k in ("c", "W", "groups", "merged", "B", "Lmax", "max_tasks", "max_segments", "n_sorted")}
    res.update(M=M, K=sum(int(w) << (32 * i) for i, w in enumerate(info.K)), offsets=offsets[:M + 1].copy(), task_off=task_off[:M + 1].copy(),
               heavy=heavy[:M + 1].copy(), sorted=srt[:info.n_sorted].copy())
    return status, res


def window_table_lab(lb: "Lib", ctx, g2: bool, points: np.ndarray, c: int, W: int, fill: int = 0xDEADBEEFDEADBEEF):
    """g16_dev_window_table_lab (test hook): the key loader's window-table builder on caller-made points.
    points: uint64 [n, affine words] in the ABI's form.  Returns (status, uint64 [W, n, affine words]: row j of point i is
    2^(c j) P_i, canonical x R' and y R' in the packed form's words, an identity row all zero).  The buffer is pre-filled with
    `fill`, so what the call did not write shows."""
    points = np.ascontiguousarray(points, dtype=np.uint64)
    assert points.ndim == 2
    out = np.full((max(W, 0), points.shape[0], points.shape[1]), fill, dtype=np.uint64)
    status = lb.c.g16_dev_window_table_lab(ctx, int(g2), ptr64(points), points.shape[0], c, W, ptr64(out))
    return status, out


PVK_WINDOWS, PVK_DIGITS = 64, 15   # a prepared key's window tables: [base][window][digit - 1]


def _input_rows(inputs, num_public: int) -> np.ndarray:
    """n rows of num_public Fr (Montgomery limbs) as uint64 [n, num_public, 4]"""
    x = np.ascontiguousarray(inputs, dtype=np.uint64)
    assert x.ndim == 3 and x.shape[1:] == (num_public, 4), "expected uint64 [n, num_public, 4]"
    return x


def dev_pvk_tables(lb: "Lib", ctx, pvk, num_public: int, fq_limbs: int, device_index: int = 0, fill: int = 0xDEADBEEFDEADBEEF):
    """g16_dev_pvk_tables (test hook): the resident window tables of a prepared key's copy `device_index`.
    ctx, pvk: the raw handles.  Returns (status, uint64 [num_public, 64, 15, 2 * fq_limbs]: entry [j, w, d - 1] is
    d * 16^w * gamma_abc_g1[j + 1] in the ABI's affine form); the buffer is pre-filled with `fill`."""
    out = np.full((num_public, PVK_WINDOWS, PVK_DIGITS, 2 * fq_limbs), fill, dtype=np.uint64)
    status = lb.c.g16_dev_pvk_tables(ctx, pvk, device_index, ptr64(out))
    return status, out


def host_pvk_tables(lb: "Lib", curve_id: int, vk_view, num_public: int, fq_limbs: int, fill: int = 0xDEADBEEFDEADBEEF):
    """g16_host_pvk_tables (test hook): the same tables built on the CPU by the table kernel's own function.  vk_view: a VkViewC."""
    out = np.full((num_public, PVK_WINDOWS, PVK_DIGITS, 2 * fq_limbs), fill, dtype=np.uint64)
    status = lb.c.g16_host_pvk_tables(curve_id, C.byref(vk_view), ptr64(out))
    return status, out


def dev_prepare_inputs(lb: "Lib", ctx, pvk, inputs, num_public: int, fq_limbs: int, fill: int = 0xDEADBEEFDEADBEEF):
    """g16_dev_prepare_inputs (test hook): one GPU lane per row of `inputs` (uint64 [n, num_public, 4]) through prepare_inputs_tab on
    the key's resident tables.  Returns (status, uint64 [n, 2 * fq_limbs] affine points, pre-filled with `fill`)."""
    x = _input_rows(inputs, num_public)
    out = np.full((x.shape[0], 2 * fq_limbs), fill, dtype=np.uint64)
    status = lb.c.g16_dev_prepare_inputs(ctx, pvk, ptr64(x) if x.size else None, num_public, x.shape[0], ptr64(out))
    return status, out


def host_prepare_inputs(lb: "Lib", curve_id: int, vk_view, inputs, num_public: int, fq_limbs: int, fill: int = 0xDEADBEEFDEADBEEF):
    """g16_host_prepare_inputs (test hook): the same on the CPU, tables built by the table kernel's own function"""
    x = _input_rows(inputs, num_public)
    out = np.full((x.shape[0], 2 * fq_limbs), fill, dtype=np.uint64)
    status = lb.c.g16_host_prepare_inputs(curve_id, C.byref(vk_view), ptr64(x) if x.size else None, num_public, x.shape[0], ptr64(out))
    return status, out


_LIB: Optional[Lib] = None


def lib() -> Lib:
    global _LIB
    if _LIB is None:
        _LIB = Lib()
    return _LIB
