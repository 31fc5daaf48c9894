"""Host-side mirror of ark-groth16's prover interface over the C ABI (see package docstring).

Data is held exactly as the Rust side holds it: numpy uint64 arrays of little-endian Montgomery
limbs (``Fr`` = 4 limbs; ``Fq`` = 6 / 4 limbs for BLS12-381 / BN254), affine points as
``x|y`` (G1) or ``x.c0 x.c1 y.c0 y.c1`` (G2), the identity as all-zero limbs.
"""
from __future__ import annotations

import ctypes as C
import secrets
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .binding import (CURVE_ID, FQ_LIMBS, QAP_CIRCOM, QAP_LIBSNARK, CeremonyInfoC, CeremonyTimingsC, CheckResultC, CsrViewC, G16Error, KeyFoldC, KeycheckTimingsC, LagrangeSrsViewC, LagrangeTimingsC, ParamsViewC, PartialC, Phase1TimingsC, PkBytesInfoC, PkInfoC, PkViewC, ProofC, QueryC, SrsTimingsC, SrsViewC, TauContributionC, TimingsC,
                      ToxicWasteC, lib, ptr32, ptr64, u64p)

_MODULUS_R = {
    "bls12_381": 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001,
    "bn254": 21888242871839275222246405745257275088548364400416034343698204186575808495617,
}

_MODULUS_Q = {
    "bls12_381": 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB,
    "bn254": 21888242871839275222246405745257275088696311157297823662689037894645226208583,
}
# the curves' standard generators (x, y; G2 coordinates as (c0, c1)): IETF pairing-friendly-curves draft / EIP-197
_GENERATORS = {
    "bls12_381": (
        (0x17F1D3A73197D7942695638C4FA9AC0FC3688C4F9774B905A14E3A3F171BAC586C55E83FF97A1AEFFB3AF00ADB22C6BB,
         0x08B3F481E3AAA0F1A09E30ED741D8AE4FCF5E095D5D00AF600DB18CB2C04B3EDD03CC744A2888AE40CAA232946C5E7E1),
        ((0x024AA2B2F08F0A91260805272DC51051C6E47AD4FA403B02B4510B647AE3D1770BAC0326A805BBEFD48056C8C121BDB8,
          0x13E02B6052719F607DACD3A088274F65596BD0D09920B61AB5DA61BBDC7F5049334CF11213945D57E5AC7D055D042B7E),
         (0x0CE5D527727D6E118CC9CDC6DA2E351AADFD9BAA8CBDD3A76D429A695160D12C923AC9CC3BACA289E193548608B82801,
          0x0606C4A02EA734CC32ACD2B02BC28B99CB3E287E85A763AF267492AB572E99AB3F370D275CEC1DA1AAA9075FF05F79BE))),
    "bn254": (
        (1, 2),
        ((10857046999023057135944570762232829481370756359578518086990519993285655852781,
          11559732032986387107991004021392285783925812861821192530917403151452391805634),
         (8495653923123431417604973247489272438418190587263600148770280649306958101930,
          4082367875863433681332203403145435568316851327593401208105741076214120093531))),
}


def _c(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.uint64)


def _limbs(v: int, n: int) -> List[int]:
    return [(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(n)]


def _fq_mont(curve: str, coords: Sequence[int]) -> np.ndarray:
    """integers mod q -> concatenated Montgomery limbs (the in-memory form of an affine point's coordinates)"""
    L, q = FQ_LIMBS[curve], _MODULUS_Q[curve]
    return np.array([w for x in coords for w in _limbs((x << (64 * L)) % q, L)], dtype=np.uint64)


def _rand_fr(curve: str, rng=None, nonzero: bool = False) -> np.ndarray:
    """F::rand(rng) as Montgomery limbs; rng: anything with getrandbits (random.Random), default the OS source"""
    p = _MODULUS_R[curve]
    while True:
        v = (rng.getrandbits(512) if rng is not None else secrets.randbits(512)) % p
        if v or not nonzero:
            return np.array(_limbs((v << 256) % p, 4), dtype=np.uint64)


@dataclass
class ConstraintMatrices:
    """ark_relations::r1cs::ConstraintMatrices flattened to CSR (row_ptr u64, col u32, val Fr)."""

    num_instance_variables: int
    num_witness_variables: int
    num_constraints: int
    a: Tuple[np.ndarray, np.ndarray, np.ndarray]
    b: Tuple[np.ndarray, np.ndarray, np.ndarray]
    c: Tuple[np.ndarray, np.ndarray, np.ndarray]

    @staticmethod
    def from_rows(curve: str, num_instance: int, num_witness: int, rows_a, rows_b, rows_c) -> "ConstraintMatrices":
        """rows: Vec<Vec<(F, usize)>> with F given as 4-limb Montgomery arrays."""
        def conv(rows):
            rp = np.zeros(len(rows) + 1, dtype=np.uint64)
            cols, vals = [], []
            for i, row in enumerate(rows):
                for coeff, idx in row:
                    cols.append(idx)
                    vals.append(np.asarray(coeff, dtype=np.uint64))
                rp[i + 1] = len(cols)
            val = np.stack(vals) if vals else np.zeros((0, 4), dtype=np.uint64)
            return rp, np.asarray(cols, dtype=np.uint32), _c(val)
        return ConstraintMatrices(num_instance, num_witness, len(rows_a), conv(rows_a), conv(rows_b), conv(rows_c))


@dataclass
class ProvingKey:
    """src/data_structures.rs:125-143 (vk fields the prover reads are flattened in)."""

    curve: str
    alpha_g1: np.ndarray
    beta_g1: np.ndarray
    delta_g1: np.ndarray
    beta_g2: np.ndarray
    delta_g2: np.ndarray
    a_query: np.ndarray
    b_g1_query: np.ndarray
    b_g2_query: np.ndarray
    h_query: np.ndarray
    l_query: np.ndarray
    # the rest of the VerifyingKey (data_structures.rs:28-41); the prover never reads these
    gamma_g2: Optional[np.ndarray] = None
    gamma_abc_g1: Optional[np.ndarray] = None


@dataclass
class SRS:
    """A phase-1 structured reference string (powers of tau) as g16_srs_view takes it: affine Montgomery limbs, one point per row.
    tau_g1[i] = tau^i G1 (a domain of n points needs 2n - 1 of them), tau_g2[i] = tau^i G2, alpha_tau_g1[i] = alpha tau^i G1,
    beta_tau_g1[i] = beta tau^i G1 (n each), beta_g2 = beta G2.  Longer arrays are fine: the prefix is used."""

    curve: str
    tau_g1: np.ndarray
    tau_g2: np.ndarray
    alpha_tau_g1: np.ndarray
    beta_tau_g1: np.ndarray
    beta_g2: np.ndarray

    def view(self):
        """(SrsViewC, the arrays it points into): hold both until the C call has returned"""
        keep = [_c(getattr(self, n)) for n in ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1", "beta_g2")]
        t1, t2, a1, b1, b2 = keep
        return SrsViewC(ptr64(t1.reshape(-1)), len(t1), ptr64(t2.reshape(-1)), len(t2), ptr64(a1.reshape(-1)), ptr64(b1.reshape(-1)),
                        min(len(a1), len(b1)), ptr64(b2.reshape(-1))), keep


def _blank_key(curve: str, qap, matrices: "ConstraintMatrices") -> "ProvingKey":
    """a zeroed ProvingKey with the arrays a generator fills for these matrices"""
    L = FQ_LIMBS[curve]
    ni, nv = matrices.num_instance_variables, matrices.num_instance_variables + matrices.num_witness_variables
    need, n = matrices.num_constraints + ni, 1
    while n < need:
        n <<= 1
    g1 = lambda k: np.zeros((k, 2 * L), dtype=np.uint64)  # noqa: E731
    g2 = lambda k: np.zeros((k, 4 * L), dtype=np.uint64)  # noqa: E731
    return ProvingKey(curve, g1(1), g1(1), g1(1), g2(1), g2(1), g1(nv), g1(nv), g2(nv), g1(qap.h_query_len(n)), g1(nv - ni), g2(1), g1(ni))


def _params_view(pk: "ProvingKey") -> ParamsViewC:
    vp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    return ParamsViewC(ptr64(pk.alpha_g1), ptr64(pk.beta_g1), ptr64(pk.delta_g1), ptr64(pk.beta_g2), ptr64(pk.delta_g2), ptr64(pk.gamma_g2),
                       ptr64(pk.gamma_abc_g1), vp(pk.a_query), vp(pk.b_g1_query), vp(pk.b_g2_query), vp(pk.h_query), vp(pk.l_query), 0)


def _points_g2(curve: str, points: np.ndarray) -> bool:
    """whether an (n, width) array of affine points holds G2 points, by its width"""
    L = FQ_LIMBS[curve]
    if points.ndim != 2 or points.shape[1] not in (2 * L, 4 * L):
        raise ValueError(f"expected (n, {2 * L}) G1 or (n, {4 * L}) G2 affine points")
    return points.shape[1] == 4 * L


def _log2_exact(n: int) -> int:
    if n < 1 or n & (n - 1):
        raise ValueError("the number of points must be a power of two")
    return n.bit_length() - 1


def group_ntt_host(curve: str, points: np.ndarray, inverse: bool = False) -> np.ndarray:
    """g16_host_group_ntt: the transform of Groth16.group_ntt in plain host code (no GPU)"""
    pts = _c(points)
    out = np.zeros_like(pts)
    lb = lib()
    lb.check(lb.c.g16_host_group_ntt(CURVE_ID[curve], int(_points_g2(curve, pts)), ptr64(pts.reshape(-1)), _log2_exact(len(pts)), int(inverse),
                                     ptr64(out.reshape(-1))))
    return out


def generate_parameters_from_srs_host(curve: str, matrices: "ConstraintMatrices", srs: "SRS", qap=None) -> "ProvingKey":
    """g16_host_generate_parameters_srs: Groth16.generate_parameters_from_srs in plain host code (no GPU; for small circuits)"""
    qap = qap or LibsnarkReduction
    if srs.curve != curve:
        raise ValueError("the SRS is for another curve")
    pk = _blank_key(curve, qap, matrices)
    out = _params_view(pk)
    views, keep = _csr_views(matrices)
    sv, skeep = srs.view()
    ni = matrices.num_instance_variables
    lb = lib()
    lb.check(lb.c.g16_host_generate_parameters_srs(CURVE_ID[curve], views, ni, matrices.num_constraints, ni + matrices.num_witness_variables,
                                                   qap.QAP_ID, C.byref(sv), C.byref(out)))
    return pk


# ---- the Lagrange form of an SRS and the key from it (g16_srs_lagrange / g16_generate_parameters_lagrange; libg16_lagrange.so) ----
LAGRANGE_ARRAYS = ("u_g1", "alpha_u_g1", "beta_u_g1", "u_g2", "h_g1", "tau_g1_0", "alpha_g1_0", "beta_g1_0", "tau_g2_0", "beta_g2")


@dataclass
class LagrangeSRS:
    """The Lagrange form of an SRS for one domain of 2^log_n points and one reduction (g16_lagrange_srs_view): what snarkjs'
    `powersoftau prepare phase2` leaves.  u_g1, alpha_u_g1, beta_u_g1, u_g2: the inverse transforms over the group of the first n
    points of tau_g1, alpha_tau_g1, beta_tau_g1, tau_g2; h_g1: the delta = 1 h_query of the reduction; the five single points the
    key copies.  Made once by Groth16.prepare_srs, kept with save / load, it serves every circuit of that domain."""

    curve: str
    log_n: int
    qap: int   # QAP_LIBSNARK or QAP_CIRCOM (R1CSToQAP.QAP_ID)
    u_g1: np.ndarray
    alpha_u_g1: np.ndarray
    beta_u_g1: np.ndarray
    u_g2: np.ndarray
    h_g1: np.ndarray
    tau_g1_0: np.ndarray
    alpha_g1_0: np.ndarray
    beta_g1_0: np.ndarray
    tau_g2_0: np.ndarray
    beta_g2: np.ndarray

    @staticmethod
    def blank(curve: str, log_n: int, qap) -> "LagrangeSRS":
        """zeroed arrays of the shapes a domain of 2^log_n points and the reduction `qap` need"""
        L, n = FQ_LIMBS[curve], 1 << log_n
        g1 = lambda k: np.zeros((k, 2 * L), dtype=np.uint64)  # noqa: E731
        g2 = lambda k: np.zeros((k, 4 * L), dtype=np.uint64)  # noqa: E731
        return LagrangeSRS(curve, log_n, qap.QAP_ID, g1(n), g1(n), g1(n), g2(n), g1(qap.h_query_len(n)), g1(1), g1(1), g1(1), g2(1), g2(1))

    def view(self):
        """(LagrangeSrsViewC, the arrays it points into): hold both until the C call has returned.  The shapes are held against
        log_n and qap here: the C view carries no lengths"""
        L, n = FQ_LIMBS[self.curve], 1 << self.log_n
        n_h = n if self.qap == QAP_CIRCOM else n - 1
        want = {"u_g1": (n, 2 * L), "alpha_u_g1": (n, 2 * L), "beta_u_g1": (n, 2 * L), "u_g2": (n, 4 * L), "h_g1": (n_h, 2 * L),
                "tau_g1_0": (1, 2 * L), "alpha_g1_0": (1, 2 * L), "beta_g1_0": (1, 2 * L), "tau_g2_0": (1, 4 * L), "beta_g2": (1, 4 * L)}
        keep = [_c(getattr(self, k)) for k in LAGRANGE_ARRAYS]
        for k, a in zip(LAGRANGE_ARRAYS, keep):
            if a.size != want[k][0] * want[k][1]:
                raise ValueError(f"LagrangeSRS.{k} has shape {a.shape}, a domain of 2^{self.log_n} points needs {want[k]}")
        empty = np.zeros(1, dtype=np.uint64)   # behind an array of no points (h_g1 of a one-point Libsnark domain): never read or written
        ptr = lambda a: ptr64(a.reshape(-1) if a.size else empty)  # noqa: E731
        return LagrangeSrsViewC(*[ptr(a) for a in keep], self.log_n, self.qap), keep + [empty]

    def save(self, path):
        """one .npz holding the curve, log_n, qap and the arrays (np.savez appends .npz to a name without it)"""
        np.savez(path, curve=np.array(self.curve), log_n=np.array(self.log_n, dtype=np.int64), qap=np.array(self.qap, dtype=np.int64),
                 **{k: _c(getattr(self, k)) for k in LAGRANGE_ARRAYS})

    @staticmethod
    def load(path) -> "LagrangeSRS":
        with np.load(path, allow_pickle=False) as z:
            return LagrangeSRS(str(z["curve"]), int(z["log_n"]), int(z["qap"]), *[np.ascontiguousarray(z[k], dtype=np.uint64) for k in LAGRANGE_ARRAYS])


def _qap_of(qap_id: int):
    return CircomReduction if qap_id == QAP_CIRCOM else LibsnarkReduction


def _domain_log(matrices: "ConstraintMatrices") -> int:
    need, log_n = matrices.num_constraints + matrices.num_instance_variables, 0
    while (1 << log_n) < need:
        log_n += 1
    return log_n


def _prepare_args(curve: str, qap, srs: "SRS", log_n, matrices):
    if srs.curve != curve:
        raise ValueError("the SRS is for another curve")
    if (log_n is None) == (matrices is None):
        raise ValueError("prepare_srs takes the domain from log_n or from the circuit's matrices: give one of the two")
    log_n = _domain_log(matrices) if matrices is not None else int(log_n)
    if log_n < 0:
        raise ValueError("log_n is negative")
    return LagrangeSRS.blank(curve, log_n, qap)


def _lagrange_key_args(curve: str, qap, matrices: "ConstraintMatrices", lagrange_srs: "LagrangeSRS"):
    """the refusals that need the object's reduction (the C view carries the Lagrange form's own): G16Error with the library's
    status for a bad argument"""
    if lagrange_srs.curve != curve:
        raise ValueError("the Lagrange SRS is for another curve")
    if lagrange_srs.qap != qap.QAP_ID:
        raise G16Error(3, f"bad argument | Lagrange SRS: prepared for the reduction qap = {lagrange_srs.qap} ({_qap_of(lagrange_srs.qap).__name__}), "
                          f"this key is derived for qap = {qap.QAP_ID} ({qap.__name__})")
    pk = _blank_key(curve, qap, matrices)
    ni = matrices.num_instance_variables
    return pk, (ni, matrices.num_constraints, ni + matrices.num_witness_variables)


def group_ntt_windowed_host(curve: str, points: np.ndarray, inverse: bool = False) -> np.ndarray:
    """g16_host_group_ntt_windowed: Groth16.group_ntt_windowed with the device kernels' own tasks run on the host (no GPU)"""
    pts = _c(points)
    out = np.zeros_like(pts)
    lb = lib()
    lb.check(lb.lag.g16_host_group_ntt_windowed(CURVE_ID[curve], int(_points_g2(curve, pts)), ptr64(pts.reshape(-1)), _log2_exact(len(pts)),
                                                int(inverse), ptr64(out.reshape(-1))))
    return out


def prepare_srs_host(curve: str, srs: "SRS", log_n: Optional[int] = None, matrices: Optional["ConstraintMatrices"] = None, qap=None) -> "LagrangeSRS":
    """g16_host_srs_lagrange: Groth16.prepare_srs in plain host code (no GPU; for small domains)"""
    qap = qap or LibsnarkReduction
    out = _prepare_args(curve, qap, srs, log_n, matrices)
    sv, skeep = srs.view()
    lv, lkeep = out.view()
    lb = lib()
    lb.check(lb.lag.g16_host_srs_lagrange(CURVE_ID[curve], C.byref(sv), out.log_n, qap.QAP_ID, C.byref(lv)))
    return out


def generate_parameters_from_lagrange_host(curve: str, matrices: "ConstraintMatrices", lagrange_srs: "LagrangeSRS", qap=None) -> "ProvingKey":
    """g16_host_generate_parameters_lagrange: Groth16.generate_parameters_from_lagrange in plain host code (no GPU)"""
    qap = qap or LibsnarkReduction
    pk, (ni, nc, nv) = _lagrange_key_args(curve, qap, matrices, lagrange_srs)
    out = _params_view(pk)
    views, keep = _csr_views(matrices)
    lv, lkeep = lagrange_srs.view()
    lb = lib()
    lb.check(lb.lag.g16_host_generate_parameters_lagrange(CURVE_ID[curve], views, ni, nc, nv, C.byref(lv), C.byref(out)))
    return pk


# ---- ceremony checks (g16_rlc_sums / g16_srs_check / g16_params_check_delta) ----
SRS_CHECK_FLAGS = {1: "BAD_POINT", 2: "TAU_G1", 4: "TAU_G2", 8: "ALPHA", 16: "BETA", 32: "BETA_G2"}
KEY_CHECK_FLAGS = {1: "BAD_POINT", 2: "FIXED_PART", 4: "DELTA", 8: "L", 16: "H"}
SRS_ARRAYS = ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1", "beta_g2")
KEY_POINT_ARRAYS = ("delta_g1", "delta_g2", "l_query", "h_query")
KEY_FIXED_ARRAYS = ("alpha_g1", "beta_g1", "beta_g2", "gamma_g2", "gamma_abc_g1", "a_query", "b_g1_query", "b_g2_query")
BAD_POINT_REASONS = {2: "off the curve", 3: "outside the prime-order subgroup", 4: "the identity"}


@dataclass
class CeremonyResult:
    """g16_ceremony_info: what check_srs / check_delta_contribution found.  Falsy when any flag is set.  `failed`: the names of the
    set flags; `array` / `index`: the first bad point (BAD_POINT) or the first differing point of the fixed part (FIXED_PART), else
    None; `reason`: 2 off the curve, 3 outside the subgroup, 4 the identity (BAD_POINT), else 0"""

    flags: int
    failed: Tuple[str, ...]
    array: Optional[str]
    index: Optional[int]
    reason: int

    @property
    def ok(self) -> bool:
        return self.flags == 0

    def __bool__(self) -> bool:
        return self.flags == 0

    @staticmethod
    def from_info(info: CeremonyInfoC, names: dict, point_arrays, fixed_arrays=()) -> "CeremonyResult":
        flags = int(info.flags)
        failed = tuple(name for bit, name in names.items() if flags & bit)
        array = index = None
        if flags & 1:
            array, index = point_arrays[info.bad_array], int(info.bad_index)
        elif fixed_arrays and flags & 2:
            array, index = fixed_arrays[info.bad_array], int(info.bad_index)
        return CeremonyResult(flags, failed, array, index, int(info.bad_reason))


class BadSRS(ValueError):
    """generate_parameters_from_srs(check=True) met an SRS that fails check_srs; `.result` is the CeremonyResult"""

    def __init__(self, result: CeremonyResult):
        where = f" ({result.array}[{result.index}] is {BAD_POINT_REASONS.get(result.reason, '?')})" if result.array else ""
        super().__init__("the SRS is not well formed: " + ", ".join(result.failed) + where)
        self.result = result


def _coeffs128(coeffs) -> Optional[np.ndarray]:
    """128-bit coefficients as an (n, 2) array of little-endian words: from such an array, or from Python integers"""
    if coeffs is None:
        return None
    if isinstance(coeffs, np.ndarray) and coeffs.dtype == np.uint64:
        return _c(coeffs).reshape(-1, 2)
    vals = [int(v) for v in coeffs]
    if any(v < 0 or v >> 128 for v in vals):
        raise ValueError("a coefficient does not fit 128 bits")
    return np.array([[v & 0xFFFFFFFFFFFFFFFF, v >> 64] for v in vals], dtype=np.uint64).reshape(-1, 2)


def _coeff_args(coeffs):
    co = _coeffs128(coeffs)
    return co, (None if co is None else ptr64(co.reshape(-1))), (0 if co is None else len(co))


def _key_for_check(pk: "ProvingKey") -> "ProvingKey":
    if pk.gamma_g2 is None or pk.gamma_abc_g1 is None:
        raise ValueError("the key check compares the whole key: gamma_g2 and gamma_abc_g1 are missing")
    names = ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "delta_g2", "a_query", "b_g1_query", "b_g2_query", "h_query", "l_query", "gamma_g2",
             "gamma_abc_g1")
    return ProvingKey(pk.curve, *[_c(getattr(pk, n)) for n in names])


def _delta_check_args(curve: str, before: "ProvingKey", after: "ProvingKey"):
    if before.curve != curve or after.curve != curve:
        raise ValueError("proving key is for another curve")
    b, a = _key_for_check(before), _key_for_check(after)
    for n in KEY_FIXED_ARRAYS + KEY_POINT_ARRAYS:
        if getattr(b, n).shape != getattr(a, n).shape:
            raise ValueError(f"the two keys differ in shape: {n} is {getattr(b, n).shape} before and {getattr(a, n).shape} after")
    return b, a, (len(b.a_query), len(b.gamma_abc_g1), len(b.l_query), len(b.h_query))


def rlc_plan(n_coeffs: int) -> dict:
    """g16_rlc_plan: how n_coeffs 128-bit coefficients are sorted -- window_bits, windows, chunk (coefficients per histogram / scatter
    workgroup), segment (entries one bucket-pass lane walks)"""
    out = np.zeros(4, dtype=np.uint32)
    lb = lib()
    lb.check(lb.cer.g16_rlc_plan(n_coeffs, ptr32(out)))
    return dict(window_bits=int(out[0]), windows=int(out[1]), chunk=int(out[2]), segment=int(out[3]))


def rlc_sums_host(curve: str, points: np.ndarray, coeffs) -> Tuple[np.ndarray, np.ndarray]:
    """g16_host_rlc_sums: Groth16.rlc_sums by plain scalar multiplications and additions (no GPU)"""
    pts = _c(points)
    lo, hi = np.zeros(pts.shape[1], dtype=np.uint64), np.zeros(pts.shape[1], dtype=np.uint64)
    co, cp, _ = _coeff_args(coeffs)
    if co is not None and len(co) < len(pts) - 1:
        raise ValueError(f"{len(pts)} points need {len(pts) - 1} coefficients")
    lb = lib()
    lb.check(lb.cer.g16_host_rlc_sums(CURVE_ID[curve], int(_points_g2(curve, pts)), ptr64(pts.reshape(-1)), len(pts), cp, ptr64(lo), ptr64(hi)))
    return lo, hi


def check_srs_host(curve: str, srs: "SRS", coeffs=None) -> CeremonyResult:
    """g16_host_srs_check: Groth16.check_srs in plain host code (no GPU; for small SRS)"""
    if srs.curve != curve:
        raise ValueError("the SRS is for another curve")
    sv, keep = srs.view()
    co, cp, nco = _coeff_args(coeffs)
    info = CeremonyInfoC()
    lb = lib()
    lb.check(lb.cer.g16_host_srs_check(CURVE_ID[curve], C.byref(sv), cp, nco, C.byref(info)))
    return CeremonyResult.from_info(info, SRS_CHECK_FLAGS, SRS_ARRAYS)


def check_delta_contribution_host(curve: str, before: "ProvingKey", after: "ProvingKey", coeffs=None) -> CeremonyResult:
    """g16_host_params_check_delta: Groth16.check_delta_contribution in plain host code (no GPU; for small keys)"""
    b, a, (nv, ni, nl, nh) = _delta_check_args(curve, before, after)
    co, cp, nco = _coeff_args(coeffs)
    info = CeremonyInfoC()
    bv, av = _params_view(b), _params_view(a)
    lb = lib()
    lb.check(lb.cer.g16_host_params_check_delta(CURVE_ID[curve], C.byref(bv), C.byref(av), nv, ni, nl, nh, cp, nco, C.byref(info)))
    return CeremonyResult.from_info(info, KEY_CHECK_FLAGS, KEY_POINT_ARRAYS, KEY_FIXED_ARRAYS)


# ---- phase 1 (g16_batch_scalar_mul / g16_srs_contribute / g16_srs_check_contribution; libg16_phase1.so) ----
TAU_CHECK_FLAGS = {**SRS_CHECK_FLAGS, 64: "SHAPE", 128: "TAU_RATIO", 256: "ALPHA_RATIO", 512: "BETA_RATIO"}
TAU_ARRAYS = SRS_ARRAYS + ("pub_tau_g2", "pub_alpha_g2", "pub_beta_g2", "before")


@dataclass
class TauContribution:
    """g16_tau_contribution: a phase-1 contributor's public record -- tau' g2, alpha' g2, beta' g2 with g2 = tau_g2[0] of the SRS the
    contribution was made to; one G2 affine point each (Montgomery limbs)"""

    curve: str
    tau_g2: np.ndarray
    alpha_g2: np.ndarray
    beta_g2: np.ndarray

    def view(self):
        """(TauContributionC, the arrays it points into): hold both until the C call has returned"""
        keep = [_c(getattr(self, n)).reshape(-1) for n in ("tau_g2", "alpha_g2", "beta_g2")]
        return TauContributionC(*[ptr64(a) for a in keep]), keep


def _smul_args(curve: str, points: np.ndarray, scalars: np.ndarray):
    pts, sc = _c(points), _c(scalars).reshape(-1, 4)
    g2 = _points_g2(curve, pts)
    if len(sc) != len(pts):
        raise ValueError(f"{len(pts)} points need {len(pts)} scalars, got {len(sc)}")
    return pts, sc, int(g2), np.zeros_like(pts)


def batch_scalar_mul_host(curve: str, points: np.ndarray, scalars: np.ndarray, windowed: bool = False) -> np.ndarray:
    """g16_host_batch_scalar_mul: Groth16.batch_scalar_mul by plain double-and-add on the host (no GPU).  windowed=True runs the
    device kernel's own task -- signed 4-bit window, lazy 30-bit arithmetic, a lane pair emulated by its halves -- on the host instead"""
    pts, sc, g2, out = _smul_args(curve, points, scalars)
    lb = lib()
    fn = lb.ph1.g16_host_batch_scalar_mul_windowed if windowed else lb.ph1.g16_host_batch_scalar_mul
    lb.check(fn(CURVE_ID[curve], g2, ptr64(pts.reshape(-1)), ptr64(sc.reshape(-1)), len(pts), ptr64(out.reshape(-1))))
    return out


def _contribution_setup(curve: str, srs: "SRS", tau, alpha, beta):
    if srs.curve != curve:
        raise ValueError("the SRS is for another curve")
    sec = [_rand_fr(curve, nonzero=True) if s is None else _c(s).reshape(4) for s in (tau, alpha, beta)]
    new = SRS(curve, *[_c(getattr(srs, n)).copy() for n in SRS_ARRAYS])
    L = FQ_LIMBS[curve]
    pub = TauContribution(curve, *[np.zeros(4 * L, dtype=np.uint64) for _ in range(3)])
    return sec, new, pub


def contribute_tau_host(curve: str, srs: "SRS", tau=None, alpha=None, beta=None) -> Tuple["SRS", "TauContribution"]:
    """g16_host_srs_contribute: Groth16.contribute_tau in plain host code (no GPU; for small SRS)"""
    sec, new, pub = _contribution_setup(curve, srs, tau, alpha, beta)
    sv, keep = new.view()
    pv, pkeep = pub.view()
    lb = lib()
    lb.check(lb.ph1.g16_host_srs_contribute(CURVE_ID[curve], ptr64(sec[0]), ptr64(sec[1]), ptr64(sec[2]), C.byref(sv), C.byref(pv), None))
    return new, pub


def _tau_check_args(curve: str, before: "SRS", after: "SRS", contribution: "TauContribution"):
    if before.curve != curve or after.curve != curve or contribution.curve != curve:
        raise ValueError("the SRS or the contribution is for another curve")
    (bv, bkeep), (av, akeep), (pv, pkeep) = before.view(), after.view(), contribution.view()
    return bv, av, pv, (bkeep, akeep, pkeep)


def check_tau_contribution_host(curve: str, before: "SRS", after: "SRS", contribution: "TauContribution", coeffs=None) -> CeremonyResult:
    """g16_host_srs_check_contribution: Groth16.check_tau_contribution in plain host code (no GPU; for small SRS)"""
    bv, av, pv, keep = _tau_check_args(curve, before, after, contribution)
    co, cp, nco = _coeff_args(coeffs)
    info = CeremonyInfoC()
    lb = lib()
    lb.check(lb.ph1.g16_host_srs_check_contribution(CURVE_ID[curve], C.byref(bv), C.byref(av), C.byref(pv), cp, nco, C.byref(info)))
    return CeremonyResult.from_info(info, TAU_CHECK_FLAGS, TAU_ARRAYS)


# ---- the key check without the derivation (g16_params_check_derivation / g16_key_fold_from_srs; libg16_keycheck.so) ----
KEY_DERIVATION_FLAGS = {1: "BAD_POINT", 2: "FIXED", 4: "DELTA", 8: "A", 16: "B_G1", 32: "B_G2", 64: "GAMMA_ABC", 128: "L", 256: "H"}
KEY_DERIVATION_ARRAYS = ("a_query", "b_g1_query", "b_g2_query", "gamma_abc_g1", "l_query", "h_query", "delta_g1", "delta_g2")
KEY_DERIVATION_FIXED = ("alpha_g1", "beta_g1", "beta_g2", "gamma_g2")
KEY_FOLD_POINTS = ("a", "b_g1", "b_g2", "gamma_abc", "l", "h")


def _derivation_shape(curve: str, matrices: "ConstraintMatrices", srs: "SRS"):
    if srs.curve != curve:
        raise ValueError("the SRS is for another curve")
    ni = matrices.num_instance_variables
    return ni, matrices.num_constraints, ni + matrices.num_witness_variables


def _derivation_key(curve: str, qap, matrices: "ConstraintMatrices", pk: "ProvingKey") -> "ProvingKey":
    """the key as contiguous arrays, its shape held against the circuit's (ValueError: a key of another shape is not a flag)"""
    if pk.curve != curve:
        raise ValueError("proving key is for another curve")
    key = _key_for_check(pk)
    blank = _blank_key(curve, qap, matrices)
    for n in KEY_DERIVATION_ARRAYS + KEY_DERIVATION_FIXED:
        if getattr(key, n).size != getattr(blank, n).size:   # (a single point may come flat or as one row)
            raise ValueError(f"the key does not have the circuit's shape: {n} is {getattr(key, n).shape}, the circuit and this reduction "
                             f"need {getattr(blank, n).shape}")
    return key


def _fold_out(curve: str):
    L = FQ_LIMBS[curve]
    pts = {n: np.zeros(4 * L if n == "b_g2" else 2 * L, dtype=np.uint64) for n in KEY_FOLD_POINTS}
    return pts, KeyFoldC(*[ptr64(pts[n]) for n in KEY_FOLD_POINTS])


def _fold_coeffs(coeffs):
    if coeffs is None:
        raise ValueError("fold_key_from_srs is the deterministic unit: it needs explicit coefficients")
    return _coeff_args(coeffs)


def check_key_derivation_host(curve: str, matrices: "ConstraintMatrices", srs: "SRS", pk: "ProvingKey", coeffs=None, qap=None) -> CeremonyResult:
    """g16_host_params_check_derivation: Groth16.check_key_derivation in plain host code (no GPU; for small circuits)"""
    qap = qap or LibsnarkReduction
    ni, nc, nv = _derivation_shape(curve, matrices, srs)
    key = _derivation_key(curve, qap, matrices, pk)
    views, keep = _csr_views(matrices)
    sv, skeep = srs.view()
    kv = _params_view(key)
    co, cp, nco = _coeff_args(coeffs)
    info = CeremonyInfoC()
    lb = lib()
    lb.check(lb.kc.g16_host_params_check_derivation(CURVE_ID[curve], views, ni, nc, nv, qap.QAP_ID, C.byref(sv), C.byref(kv), cp, nco, C.byref(info)))
    return CeremonyResult.from_info(info, KEY_DERIVATION_FLAGS, KEY_DERIVATION_ARRAYS, KEY_DERIVATION_FIXED)


def fold_key_from_srs_host(curve: str, matrices: "ConstraintMatrices", srs: "SRS", coeffs, qap=None) -> Dict[str, np.ndarray]:
    """g16_host_key_fold_from_srs: Groth16.fold_key_from_srs in plain host code (no GPU; for small circuits)"""
    qap = qap or LibsnarkReduction
    ni, nc, nv = _derivation_shape(curve, matrices, srs)
    views, keep = _csr_views(matrices)
    sv, skeep = srs.view()
    co, cp, nco = _fold_coeffs(coeffs)
    pts, out = _fold_out(curve)
    lb = lib()
    lb.check(lb.kc.g16_host_key_fold_from_srs(CURVE_ID[curve], views, ni, nc, nv, qap.QAP_ID, C.byref(sv), cp, nco, C.byref(out)))
    return pts


@dataclass
class Proof:
    """src/data_structures.rs:8-16; affine Montgomery limbs."""

    a: np.ndarray
    b: np.ndarray
    c: np.ndarray

    def __eq__(self, o):
        return (self.a == o.a).all() and (self.b == o.b).all() and (self.c == o.c).all()

    def flat(self) -> np.ndarray:
        return np.concatenate([self.a, self.b, self.c])


@dataclass
class CheckResult:
    """g16_check_result: what cs.is_satisfied() / cs.which_is_unsatisfied() say of (matrices, assignment).  `first_row` is the lowest
    failing row, None when every row holds; a, b, c are that row's <A_row, z>, <B_row, z>, <C_row, z> as Montgomery limbs (zero when
    nothing fails)"""

    n_unsatisfied: int
    first_row: Optional[int]
    a: np.ndarray
    b: np.ndarray
    c: np.ndarray

    @property
    def satisfied(self) -> bool:
        return self.n_unsatisfied == 0

    @staticmethod
    def from_c(res: CheckResultC) -> "CheckResult":
        first = int(res.first_row)
        return CheckResult(int(res.n_unsatisfied), None if first == 0xFFFFFFFFFFFFFFFF else first,
                           *[np.array(list(getattr(res, k)), dtype=np.uint64) for k in "abc"])

    def __eq__(self, o):
        return (self.n_unsatisfied == o.n_unsatisfied and self.first_row == o.first_row and (self.a == o.a).all() and (self.b == o.b).all()
                and (self.c == o.c).all())


def host_check_assignment(curve: str, matrices: "ConstraintMatrices", full_assignment: np.ndarray) -> CheckResult:
    """g16_host_circuit_check: the check of Groth16.check_assignment by the same row walk compiled for the host -- no GPU needed"""
    views, keep = _csr_views(matrices)
    z = _c(full_assignment)
    res = CheckResultC()
    lb = lib()
    lb.check(lb.c.g16_host_circuit_check(CURVE_ID[curve], views, matrices.num_constraints, z.ctypes.data, z.shape[0], C.byref(res)))
    return CheckResult.from_c(res)


def shard_ranges(m: int, w: int, h_len: int, num_inputs: int, idx: int, cnt: int):
    """Contiguous shard `idx` of `cnt` of the five MSM base arrays.  a / b_g1 / b_g2 (index space query[1..], length m)
    are cut identically; l (length w, index j <-> a-index j + num_inputs - 1) is cut at the matching places so that
    the library can reuse the witness bucket sort for it; h (length h_len) is cut evenly."""
    a_lo, a_hi = m * idx // cnt, m * (idx + 1) // cnt
    l_lo = min(w, max(0, a_lo - (num_inputs - 1)))
    l_hi = min(w, max(0, a_hi - (num_inputs - 1)))
    h_lo, h_hi = h_len * idx // cnt, h_len * (idx + 1) // cnt
    return dict(a=(a_lo, a_hi), l=(l_lo, l_hi), h=(h_lo, h_hi))


class _Ctx:
    def __init__(self, curve: str, device):
        """device: one HIP device id, or a sequence of them (g16_ctx_create_multi: the key is sharded over the devices inside
        the library and one g16_prove call uses all of them)"""
        self.lib = lib()
        self.curve = curve
        self.handle = C.c_void_p()
        if isinstance(device, (list, tuple)):
            ids = (C.c_int * len(device))(*[int(d) for d in device])
            self.lib.check(self.lib.c.g16_ctx_create_multi(CURVE_ID[curve], ids, len(device), C.byref(self.handle)))
        else:
            self.lib.check(self.lib.c.g16_ctx_create(CURVE_ID[curve], device, C.byref(self.handle)))
        self.num_devices = int(self.lib.c.g16_ctx_num_devices(self.handle))

    def close(self):
        if self.handle:
            self.lib.c.g16_ctx_destroy(self.handle)
            self.handle = C.c_void_p()


class _DevicePk:
    """g16_pk handle.  shard = (index, count) splits every MSM base array into contiguous ranges (base-range shards);
    shard = (index, count, "bucket") is the bucket-space shard: the whole key on every rank, rank `index` owning the buckets
    b mod count == index (g16_pk_load_bucket_shard)."""

    def __init__(self, ctx: _Ctx, pk: ProvingKey, num_inputs: int, shard=(0, 1), dist_h: bool = False):
        """dist_h: the h_query shard is this rank's block of the distributed witness map (dist_h_indices) instead of a
        contiguous range -- the form g16_prove_partial_h expects; bucket-space shard: the WHOLE h_query in the order the
        all-gathered blocks arrive in (bucket_h_indices)"""
        self.ctx = ctx
        self.handle = C.c_void_p()
        self._keep = []
        idx, cnt = shard[0], shard[1]
        bucket = len(shard) > 2 and shard[2] == "bucket"
        rg = shard_ranges(len(pk.a_query) - 1, len(pk.l_query), len(pk.h_query), num_inputs, 0 if bucket else idx, 1 if bucket else cnt)
        (a_lo, a_hi), (l_lo, l_hi), (h_lo, h_hi) = rg["a"], rg["l"], rg["h"]
        h_query = pk.h_query
        if dist_h:
            n_dom = len(pk.h_query) + 1                                  # domain size n = len(h_query) + 1 (generator.rs:168)
            sel = bucket_h_indices(n_dom, cnt) if bucket else dist_h_indices(n_dom, idx, cnt)
            h_query = pk.h_query[sel[sel < len(pk.h_query)]]            # only the very last index of the last rank is n - 1
            h_lo, h_hi = 0, len(h_query)

        def q(arr: np.ndarray, skip: int, lo: int, hi: int) -> QueryC:
            sl = _c(arr[skip + lo: skip + hi])
            self._keep.append(sl)
            return QueryC(sl.ctypes.data if len(sl) else None, hi - lo, 0 if (dist_h and arr is h_query) else lo)

        keep = [_c(x).reshape(-1) for x in (pk.alpha_g1, pk.beta_g1, pk.delta_g1, pk.beta_g2, pk.delta_g2, pk.a_query[0],
                                            pk.b_g1_query[0], pk.b_g2_query[0])]
        self._keep += keep
        view = PkViewC(*[ptr64(k) for k in keep], q(pk.a_query, 1, a_lo, a_hi), q(pk.b_g1_query, 1, a_lo, a_hi),
                       q(pk.b_g2_query, 1, a_lo, a_hi), q(h_query, 0, h_lo, h_hi), q(pk.l_query, 0, l_lo, l_hi), 0)
        if bucket:
            ctx.lib.check(ctx.lib.c.g16_pk_load_bucket_shard(ctx.handle, C.byref(view), idx, cnt, C.byref(self.handle)))
        else:
            ctx.lib.check(ctx.lib.c.g16_pk_load(ctx.handle, C.byref(view), C.byref(self.handle)))
        self._keep = []  # the library copied everything

    def rebind(self, rank: int, world: int):
        """g16_pk_rebind_bucket_shard: the same resident tables as rank `rank` of `world` (tests, --sim-shards)"""
        self.ctx.lib.check(self.ctx.lib.c.g16_pk_rebind_bucket_shard(self.handle, rank, world))

    def info(self) -> dict:
        """g16_pk_get_info: window sizes, why the key is held as plain bases if it is, bucket-shard rank / world, HBM bytes"""
        out = PkInfoC()
        self.ctx.lib.check(self.ctx.lib.c.g16_pk_get_info(self.handle, C.byref(out)))
        return out.as_dict()

    def close(self):
        if self.handle:
            self.ctx.lib.c.g16_pk_free(self.handle)
            self.handle = C.c_void_p()

    @classmethod
    def from_handle(cls, ctx: _Ctx, handle) -> "_DevicePk":
        """a g16_pk the library made some other way (g16_pk_load_bytes)"""
        self = cls.__new__(cls)
        self.ctx, self.handle, self._keep = ctx, handle, []
        return self


class DeviceProvingKey:
    """A proving key read from its bytes on the GPU (Groth16.load_proving_key_bytes, g16_pk_load_bytes): the five query arrays exist
    only as the device-resident window tables behind the handle; the host holds the head of the file -- alpha_g1, beta_g1, delta_g1,
    beta_g2, delta_g2, gamma_g2, gamma_abc_g1, so VerifyingKey.from_proving_key, prepare_verifying_key and rerandomize_proof take
    it -- and `counts` (points per section of the file, by name) and `consumed` (bytes read).  It proves on the Groth16 object that
    loaded it (or one sharing that object's device data), wherever a ProvingKey would; what needs the query arrays on the host
    (shards, prove_partial*, ShardedProver, finalize_host, proving_key_to_bytes) raises TypeError."""

    def __init__(self, curve: str, head: dict, counts: dict, consumed: int, ctx: _Ctx, dpk: _DevicePk):
        self.curve = curve
        for name, value in head.items():
            setattr(self, name, value)
        self.counts, self.consumed = counts, consumed
        self._ctx, self._dpk = ctx, dpk

    @property
    def handle(self):
        return self._dpk.handle

    @property
    def resident(self) -> bool:
        return bool(self._dpk.handle)


def _host_key(pk, what: str):
    """refuse a DeviceProvingKey where the query arrays are read on the host"""
    if isinstance(pk, DeviceProvingKey):
        raise TypeError(f"{what} reads the key's query arrays on the host; a DeviceProvingKey (load_proving_key_bytes) holds them on "
                        "the GPU only, as window tables: load the key with proving_key_from_bytes for this")
    return pk


def dist_h_indices(n: int, rank: int, world: int) -> np.ndarray:
    """h coefficients rank `rank` of `world` holds after the distributed witness map (g16_dwm_*): the BLOCK indices
    (rank * blk + j) + M * k1, j < blk = M / world, k1 < world, M = n / world, in the order [k1][j] -- the order its shard of
    h_query has to be gathered in (include/g16_mi355x.h)."""
    M = n // world
    blk = M // world
    return ((rank * blk + np.arange(blk, dtype=np.int64))[None, :] + (M * np.arange(world, dtype=np.int64))[:, None]).reshape(-1)


def bucket_h_indices(n: int, world: int) -> np.ndarray:
    """h coefficients in the order an all-gather of the ranks' blocks of the distributed witness map leaves them in: rank 0's
    block (dist_h_indices), rank 1's, ... -- the order a bucket-space shard's h_query is loaded in, since there every rank
    runs the h MSM over ALL coefficients (and 1 / world of the buckets)"""
    return np.concatenate([dist_h_indices(n, q, world) for q in range(world)])


def _csr_views(m: "ConstraintMatrices"):
    """CsrViewC[3] over the three matrices plus the arrays the views point into.  A ctypes structure keeps only the raw
    address: when a matrix arrives with another dtype or layout (e.g. scipy's int64 indptr) the normalised copy made here
    is what the library reads, so the caller must hold the returned list until the C call has returned."""
    keep = [(np.ascontiguousarray(x[0], dtype=np.uint64), np.ascontiguousarray(x[1], dtype=np.uint32), _c(x[2])) for x in (m.a, m.b, m.c)]
    views = (CsrViewC * 3)(*[CsrViewC(ptr64(rp), ptr32(col), ptr64(val)) for rp, col, val in keep])
    return views, keep


class _DeviceCircuit:
    def __init__(self, ctx: _Ctx, m: ConstraintMatrices, qap_id: int = QAP_LIBSNARK):
        self.ctx = ctx
        self.handle = C.c_void_p()
        self.num_variables = m.num_instance_variables + m.num_witness_variables
        self._has_c = qap_id == QAP_LIBSNARK
        views, self._keep = _csr_views(m)
        if qap_id == QAP_LIBSNARK:
            ctx.lib.check(ctx.lib.c.g16_circuit_load(ctx.handle, views, m.num_instance_variables, m.num_constraints, self.num_variables,
                                                     C.byref(self.handle)))
        else:
            ctx.lib.check(ctx.lib.c.g16_circuit_load_qap(ctx.handle, views, m.num_instance_variables, m.num_constraints, self.num_variables,
                                                         qap_id, C.byref(self.handle)))

    def attach_c(self, m: ConstraintMatrices):
        """g16_circuit_attach_c: bring a Circom circuit's C matrix to the device, for the satisfaction check alone (once; nothing
        happens on a Libsnark circuit, which holds C since its load)"""
        if self._has_c:
            return
        rp, col, val = (np.ascontiguousarray(m.c[0], dtype=np.uint64), np.ascontiguousarray(m.c[1], dtype=np.uint32), _c(m.c[2]))
        if len(rp) != m.num_constraints + 1:   # the C view carries no row count: the one place that can compare it
            raise G16Error(3, f"bad argument | C has {len(rp) - 1} rows, the circuit {m.num_constraints}")
        view = CsrViewC(ptr64(rp), ptr32(col), ptr64(val))
        self.ctx.lib.check(self.ctx.lib.c.g16_circuit_attach_c(self.ctx.handle, self.handle, C.byref(view)))
        self._has_c = True

    @property
    def qap(self) -> int:
        """g16_circuit_qap: the reduction the device copy was loaded for"""
        return int(self.ctx.lib.c.g16_circuit_qap(self.handle))

    @property
    def domain_size(self) -> int:
        return int(self.ctx.lib.c.g16_circuit_domain_size(self.handle))

    def close(self):
        if self.handle:
            self.ctx.lib.c.g16_circuit_free(self.handle)
            self.handle = C.c_void_p()


class R1CSToQAP:
    """trait R1CSToQAP (src/r1cs_to_qap.rs:71-120): what the two reductions share.  Not a reduction itself -- Groth16(qap=...) takes one
    of the two sibling classes below, which differ in QAP_ID alone."""

    QAP_ID: Optional[int] = None

    @classmethod
    def witness_map_from_matrices(cls, prover: "Groth16", matrices: ConstraintMatrices, num_inputs: int, num_constraints: int,
                                  full_assignment: np.ndarray) -> np.ndarray:
        """the map on the GPU; `prover` must be a Groth16 over this reduction (the device circuit is loaded for one)"""
        if prover.qap.QAP_ID != cls.QAP_ID:
            raise ValueError(f"the prover was made for {prover.qap.__name__}, not {cls.__name__}")
        return prover.witness_map_from_matrices(matrices, num_inputs, num_constraints, full_assignment)

    @classmethod
    def h_query_len(cls, domain_size: int) -> int:
        """bases in h_query for a domain of that size (g16_h_query_len)"""
        return int(lib().c.g16_h_query_len(cls.QAP_ID, domain_size))

    @classmethod
    def h_query_scalars(cls, curve: str, domain_size: int, t: np.ndarray, delta_inverse: np.ndarray) -> np.ndarray:
        """QAP::h_query_scalars(domain_size - 1, t, zt, delta_inverse) on the host (g16_host_h_query_scalars: the code setup runs;
        zt = t^n - 1 is computed there): (h_query_len, 4) Montgomery limbs"""
        out = np.zeros((cls.h_query_len(domain_size), 4), dtype=np.uint64)
        lb = lib()
        lb.check(lb.c.g16_host_h_query_scalars(CURVE_ID[curve], cls.QAP_ID, domain_size, ptr64(_c(t).reshape(4)),
                                               ptr64(_c(delta_inverse).reshape(4)), ptr64(out) if out.size else ptr64(np.zeros(4, dtype=np.uint64))))
        return out


class LibsnarkReduction(R1CSToQAP):
    """R1CSToQAP default reduction (src/r1cs_to_qap.rs:123-248): h = the coefficients of (A.B - C) / Z, h_query = n - 1 bases."""

    QAP_ID = QAP_LIBSNARK


class CircomReduction(R1CSToQAP):
    """ark-circom's CircomReduction, the R1CSToQAP implementor snarkjs-compatible keys are made for (restated from its published
    source, not pinned against it): h = the n evaluations of A.B - C on the odd coset of the 2n-point domain -- c = a .* b (the C
    matrix is not read), each of a, b, c through ifft, * rho^i, fft, then a.b - c -- and h_query = n bases, the odd-indexed entries
    of the size-2n inverse transform of delta^-1 t^i.  instance_map_with_evaluation is the Libsnark one.  One GPU per context:
    a multi-device context and the distributed witness map refuse a Circom circuit."""

    QAP_ID = QAP_CIRCOM


class Groth16:
    """``Groth16::<E, QAP>`` prover methods for E in {Bls12_381, Bn254} and QAP in {LibsnarkReduction (the default), CircomReduction}
    on one MI355X (``device=0``) or on several GPUs of the node behind the same calls (``device=[0, 1, ...]``: the library shards the
    key and folds the partial sums; Libsnark only).  The reduction chosen here drives circuit loading, generate_parameters* / setup
    and every create_proof* / prove.

    Device-resident copies of proving keys and constraint matrices are cached per object
    (they are per-circuit constants, like ``&pk`` in the reference)."""

    def __init__(self, curve: str = "bls12_381", device=0, qap=LibsnarkReduction):
        if curve not in CURVE_ID:
            raise ValueError(f"unsupported curve {curve}")
        if qap not in (LibsnarkReduction, CircomReduction):
            raise ValueError("qap is LibsnarkReduction or CircomReduction")
        self.curve = curve
        self.qap = qap
        self._ctx = _Ctx(curve, device)
        self._pks: Dict[Tuple[int, Tuple[int, int]], _DevicePk] = {}
        self._byte_keys: List["DeviceProvingKey"] = []   # load_proving_key_bytes: freed by evict_pk / evict / close
        self._cks: Dict[int, _DeviceCircuit] = {}
        self._circuits_by_content: Dict[bytes, ConstraintMatrices] = {}   # create_proof_with_reduction: one upload per circuit
        self._owner: Optional["Groth16"] = None

    def share_device_data_of(self, owner: "Groth16"):
        """use the device-resident keys and circuits of another prover object on the SAME GPU instead of loading copies (the C ABI
        allows it: a g16_pk / g16_circuit is read-only during a proof and may serve every single-device context of its GPU).  Two
        objects like this, driven from two threads, are the throughput mode (`PipelinedProver`).  The owner must outlive this
        object's proofs; keys and circuits are loaded -- and evicted -- through the owner only."""
        if owner.curve != self.curve:
            raise ValueError("the two provers are for different curves")
        if owner.qap.QAP_ID != self.qap.QAP_ID:
            raise ValueError("the two provers are for different reductions")
        self._owner = owner

    # -- handles -------------------------------------------------------------------------
    def _pk(self, pk: ProvingKey, num_inputs: int, shard=(0, 1), dist_h: bool = False) -> _DevicePk:
        if self._owner is not None:
            return self._owner._pk(pk, num_inputs, shard, dist_h)
        if isinstance(pk, DeviceProvingKey):
            if tuple(shard) != (0, 1) or dist_h:
                _host_key(pk, "a shard of a key")
            if pk._ctx is not self._ctx:
                raise ValueError("this DeviceProvingKey was loaded by another Groth16 object (its tables live in that object's context)")
            if not pk.resident:
                raise ValueError("this DeviceProvingKey was evicted: its tables are gone and the host holds no query arrays to reload them")
            return pk._dpk
        if dist_h and self.qap is not LibsnarkReduction:
            # the block-order gather takes n = len(h_query) + 1 and feeds the distributed map, which is the Libsnark one
            raise ValueError("dist_h key shards (prove_partial_h, prove_partial_prepare(dist_h=True)) are for LibsnarkReduction only")
        key = (id(pk), shard) if not dist_h else (id(pk), shard, "dist_h")
        if key not in self._pks:
            if pk.curve != self.curve:
                raise ValueError("proving key is for another curve")
            # the cache entry holds a reference to pk so that id(pk) cannot be recycled while it lives
            self._pks[key] = (pk, _DevicePk(self._ctx, pk, num_inputs, shard, dist_h))
        return self._pks[key][1]

    def _ck(self, m: ConstraintMatrices, for_check: bool = False) -> _DeviceCircuit:
        """for_check: the circuit is about to be checked -- a Circom circuit, which is loaded without its C matrix, gets it now"""
        if self._owner is not None:
            return self._owner._ck(m, for_check)
        if id(m) not in self._cks:
            self._cks[id(m)] = (m, _DeviceCircuit(self._ctx, m, self.qap.QAP_ID))
        dck = self._cks[id(m)][1]
        if for_check:
            dck.attach_c(m)
        return dck

    def evict_pk(self, pk: ProvingKey, shard=(0, 1)):
        """drop the device-resident copies of one key shard -- the contiguous cut and the block-order cut of the distributed
        witness map alike (their window tables are 13x the shard).  A DeviceProvingKey has nothing else: it cannot prove afterwards"""
        if isinstance(pk, DeviceProvingKey):
            if pk._ctx is self._ctx:
                pk._dpk.close()
                self._byte_keys = [k for k in self._byte_keys if k is not pk]
            return
        for key in ((id(pk), shard), (id(pk), shard, "dist_h")):
            ent = self._pks.pop(key, None)
            if ent is not None:
                ent[1].close()

    def evict(self):
        """drop every cached device-resident key / circuit (frees their HBM) and the by-content circuit index"""
        for _, p in self._pks.values():
            p.close()
        for _, c in self._cks.values():
            c.close()
        for k in self._byte_keys:
            k._dpk.close()
        self._byte_keys = []
        self._pks, self._cks = {}, {}
        self._circuits_by_content = {}

    def close(self):
        self.evict()
        self._ctx.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- generator.rs:47-208 ----------------------------------------------------------------
    def generate_parameters_with_qap(self, matrices: ConstraintMatrices, alpha: np.ndarray, beta: np.ndarray, gamma: np.ndarray,
                                     delta: np.ndarray, g1_generator: np.ndarray, g2_generator: np.ndarray, t: np.ndarray) -> ProvingKey:
        """Groth16::generate_parameters_with_qap on the matrices of an already synthesised circuit.  Arguments as the reference's
        (toxic waste as Fr limbs, generators as affine points); `t` is what the reference draws from its rng
        (domain.sample_element_outside_domain, generator.rs:90)."""
        L = FQ_LIMBS[self.curve]
        ni, nv = matrices.num_instance_variables, matrices.num_instance_variables + matrices.num_witness_variables
        need, n = matrices.num_constraints + ni, 1
        while n < need:
            n <<= 1
        g1 = lambda k: np.zeros((k, 2 * L), dtype=np.uint64)  # noqa: E731
        g2 = lambda k: np.zeros((k, 4 * L), dtype=np.uint64)  # noqa: E731
        pk = ProvingKey(self.curve, g1(1), g1(1), g1(1), g2(1), g2(1), g1(nv), g1(nv), g2(nv), g1(self.qap.h_query_len(n)), g1(nv - ni), g2(1), g1(ni))
        tw = ToxicWasteC()
        for name, v in (("alpha", alpha), ("beta", beta), ("gamma", gamma), ("delta", delta), ("t", t)):
            getattr(tw, name)[:] = [int(x) for x in _c(v).reshape(4)]
        vp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
        out = ParamsViewC(ptr64(pk.alpha_g1), ptr64(pk.beta_g1), ptr64(pk.delta_g1), ptr64(pk.beta_g2), ptr64(pk.delta_g2), ptr64(pk.gamma_g2),
                          ptr64(pk.gamma_abc_g1), vp(pk.a_query), vp(pk.b_g1_query), vp(pk.b_g2_query), vp(pk.h_query), vp(pk.l_query), 0)
        views, keep = _csr_views(matrices)   # `keep` owns the (possibly converted) arrays until the call returns
        lb = self._ctx.lib
        if self.qap.QAP_ID == QAP_LIBSNARK:
            lb.check(lb.c.g16_generate_parameters(self._ctx.handle, views, ni, matrices.num_constraints, nv, C.byref(tw),
                                                  ptr64(_c(g1_generator).reshape(-1)), ptr64(_c(g2_generator).reshape(-1)), C.byref(out)))
        else:
            lb.check(lb.c.g16_generate_parameters_qap(self._ctx.handle, views, ni, matrices.num_constraints, nv, self.qap.QAP_ID, C.byref(tw),
                                                      ptr64(_c(g1_generator).reshape(-1)), ptr64(_c(g2_generator).reshape(-1)),
                                                      C.byref(out)))
        return pk

    # -- setup without the toxic waste: a key from a powers-of-tau SRS, then delta contributions ------------------
    def srs_from_trapdoor(self, n: int, tau: np.ndarray, alpha: np.ndarray, beta: np.ndarray, g1_generator: np.ndarray,
                          g2_generator: np.ndarray) -> SRS:
        """g16_srs_from_trapdoor -- a TEST AND BENCHMARK UTILITY: the SRS a domain of n points needs (2n - 1 powers in G1, n elsewhere)
        from known secrets, on the GPU.  A real SRS comes from a ceremony whose secrets nobody holds."""
        L = FQ_LIMBS[self.curve]
        g1 = lambda k: np.zeros((k, 2 * L), dtype=np.uint64)  # noqa: E731
        g2 = lambda k: np.zeros((k, 4 * L), dtype=np.uint64)  # noqa: E731
        srs = SRS(self.curve, g1(2 * n - 1), g2(n), g1(n), g1(n), g2(1))
        sv, keep = srs.view()
        lb = self._ctx.lib
        lb.check(lb.c.g16_srs_from_trapdoor(self._ctx.handle, ptr64(_c(tau).reshape(4)), ptr64(_c(alpha).reshape(4)), ptr64(_c(beta).reshape(4)),
                                            ptr64(_c(g1_generator).reshape(-1)), ptr64(_c(g2_generator).reshape(-1)), 2 * n - 1, n, C.byref(sv)))
        return srs

    def generate_parameters_from_srs(self, matrices: ConstraintMatrices, srs: SRS, check: bool = False) -> ProvingKey:
        """g16_generate_parameters_srs: the circuit's key from the SRS by group operations alone, for this object's reduction, with
        gamma = delta = 1 (gamma_g2 = delta_g2 = G2, delta_g1 = G1).  Nobody's secret goes in: follow it with contribute_delta, once
        per party.  After ONE contribution the key equals generate_parameters_with_qap(alpha, beta, 1, delta, g1, g2, tau) exactly.
        check=True runs check_srs first and raises BadSRS (carrying the result) before anything is derived."""
        if srs.curve != self.curve:
            raise ValueError("the SRS is for another curve")
        if check:
            res = self.check_srs(srs)
            if not res:
                raise BadSRS(res)
        pk = _blank_key(self.curve, self.qap, matrices)
        out = _params_view(pk)
        views, keep = _csr_views(matrices)
        sv, skeep = srs.view()
        ni = matrices.num_instance_variables
        lb = self._ctx.lib
        lb.check(lb.c.g16_generate_parameters_srs(self._ctx.handle, views, ni, matrices.num_constraints, ni + matrices.num_witness_variables,
                                                  self.qap.QAP_ID, C.byref(sv), C.byref(out)))
        return pk

    def contribute_delta(self, pk: ProvingKey, delta: np.ndarray) -> ProvingKey:
        """g16_params_apply_delta on a copy of the key: delta_g1, delta_g2 <- delta (.), every l_query / h_query point <- delta^-1 (.).
        `pk` itself is untouched.  UnexpectedIdentity for delta = 0."""
        _host_key(pk, "contribute_delta")
        if pk.curve != self.curve:
            raise ValueError("proving key is for another curve")
        cp = lambda a: None if a is None else _c(a).copy()  # noqa: E731
        new = ProvingKey(pk.curve, *[cp(getattr(pk, n)) for n in ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "delta_g2", "a_query", "b_g1_query",
                                                                  "b_g2_query", "h_query", "l_query", "gamma_g2", "gamma_abc_g1")])
        vp = lambda a: C.c_void_p(a.ctypes.data) if a.size else None  # noqa: E731
        view = ParamsViewC(None, None, ptr64(new.delta_g1), None, ptr64(new.delta_g2), None, None, None, None, None, vp(new.h_query),
                           vp(new.l_query), 0)
        lb = self._ctx.lib
        lb.check(lb.c.g16_params_apply_delta(self._ctx.handle, ptr64(_c(delta).reshape(4)), C.byref(view), len(new.l_query), len(new.h_query)))
        return new

    def group_ntt(self, points: np.ndarray, inverse: bool = False) -> np.ndarray:
        """g16_group_ntt: out[i] = sum_k w^(ik) points[k] over n = 2^k affine points of G1 or G2 (told apart by the row width), w the
        n-th root of the scalar transforms; inverse: w^-1 and the factor n^-1.  Natural order in and out."""
        pts = _c(points)
        out = np.zeros_like(pts)
        lb = self._ctx.lib
        lb.check(lb.c.g16_group_ntt(self._ctx.handle, int(_points_g2(self.curve, pts)), ptr64(pts.reshape(-1)), _log2_exact(len(pts)), int(inverse),
                                    ptr64(out.reshape(-1))))
        return out

    # -- the Lagrange form of an SRS: transform once, derive every circuit's key from it ------------------------------
    def prepare_srs(self, srs: SRS, log_n: Optional[int] = None, matrices: Optional[ConstraintMatrices] = None) -> "LagrangeSRS":
        """g16_srs_lagrange: the Lagrange form of `srs` for a domain of 2^log_n points -- or the domain of the circuit `matrices` --
        and this object's reduction: the four inverse transforms over the group and the delta = 1 h basis, everything of
        generate_parameters_from_srs that does not depend on the circuit.  The transforms run on the windowed scalar
        multiplication of phase 1 (group_ntt_windowed).  The SRS is not checked here (check_srs does that)."""
        out = _prepare_args(self.curve, self.qap, srs, log_n, matrices)
        sv, skeep = srs.view()
        lv, lkeep = out.view()
        lb = self._ctx.lib
        lb.check(lb.lag.g16_srs_lagrange(self._ctx.handle, C.byref(sv), out.log_n, self.qap.QAP_ID, C.byref(lv)))
        return out

    def generate_parameters_from_lagrange(self, matrices: ConstraintMatrices, lagrange_srs: "LagrangeSRS") -> ProvingKey:
        """g16_generate_parameters_lagrange: the key of generate_parameters_from_srs(matrices, srs), byte for byte, from
        prepare_srs(srs) -- the sparse products and the copies only.  G16Error for a Lagrange form of another domain or another
        reduction than the circuit's and this object's.  A Lagrange form from elsewhere needs no check of its own: a key derived
        from a bad one fails check_key_derivation against the raw SRS."""
        pk, (ni, nc, nv) = _lagrange_key_args(self.curve, self.qap, matrices, lagrange_srs)
        out = _params_view(pk)
        views, keep = _csr_views(matrices)
        lv, lkeep = lagrange_srs.view()
        lb = self._ctx.lib
        lb.check(lb.lag.g16_generate_parameters_lagrange(self._ctx.handle, views, ni, nc, nv, C.byref(lv), C.byref(out)))
        return pk

    def group_ntt_windowed(self, points: np.ndarray, inverse: bool = False) -> np.ndarray:
        """g16_group_ntt_windowed: group_ntt, bit for bit, with every butterfly's twiddle multiplication on the windowed task of
        batch_scalar_mul and affine points between the stages.  G16_LAGRANGE_CHUNK (read at every call) bounds the butterflies of
        one launch."""
        pts = _c(points)
        out = np.zeros_like(pts)
        lb = self._ctx.lib
        lb.check(lb.lag.g16_group_ntt_windowed(self._ctx.handle, int(_points_g2(self.curve, pts)), ptr64(pts.reshape(-1)), _log2_exact(len(pts)),
                                               int(inverse), ptr64(out.reshape(-1))))
        return out

    def lagrange_timings(self) -> dict:
        """g16_lagrange_get_timings: stream-event milliseconds of the last prepare_srs on this object, per array and for the h
        basis (uploads and downloads included), and of the products of the last generate_parameters_from_lagrange"""
        tm = LagrangeTimingsC()
        self._ctx.lib.check(self._ctx.lib.lag.g16_lagrange_get_timings(self._ctx.handle, C.byref(tm)))
        return tm.as_dict()

    # -- ceremony checks: is the SRS a sequence of powers, does a key descend from its predecessor ------------------
    def rlc_sums(self, points: np.ndarray, coeffs) -> Tuple[np.ndarray, np.ndarray]:
        """g16_rlc_sums: (sum_{i<n-1} rho_i X[i], sum_{i<n-1} rho_i X[i+1]) over n >= 1 affine points of G1 or G2 (told apart by the
        row width) with 128-bit coefficients rho: an (n - 1, 2) array of little-endian words, Python integers, or None for fresh ones
        from the operating system.  One sort of the coefficients, both sums in one bucket-pass launch."""
        pts = _c(points)
        lo, hi = np.zeros(pts.shape[1], dtype=np.uint64), np.zeros(pts.shape[1], dtype=np.uint64)
        co, cp, _ = _coeff_args(coeffs)
        if co is not None and len(co) < len(pts) - 1:
            raise ValueError(f"{len(pts)} points need {len(pts) - 1} coefficients")
        lb = self._ctx.lib
        lb.check(lb.cer.g16_rlc_sums(self._ctx.handle, int(_points_g2(self.curve, pts)), ptr64(pts.reshape(-1)), len(pts), cp, ptr64(lo), ptr64(hi)))
        return lo, hi

    def check_srs(self, srs: SRS, coeffs=None) -> CeremonyResult:
        """g16_srs_check: every point in its subgroup and not the identity, every array a sequence of powers of the tau that tau_g2[1]
        holds, beta_g2 the beta of beta_tau_g1.  The WHOLE arrays are tested.  coeffs: as rlc_sums, at least max(array length) - 1 of
        them, fixed AFTER the SRS; None draws fresh ones.  A malformed SRS passes any one equation with probability <= 2^-128."""
        if srs.curve != self.curve:
            raise ValueError("the SRS is for another curve")
        sv, keep = srs.view()
        co, cp, nco = _coeff_args(coeffs)
        info = CeremonyInfoC()
        lb = self._ctx.lib
        lb.check(lb.cer.g16_srs_check(self._ctx.handle, C.byref(sv), cp, nco, C.byref(info)))
        return CeremonyResult.from_info(info, SRS_CHECK_FLAGS, SRS_ARRAYS)

    def check_delta_contribution(self, before: ProvingKey, after: ProvingKey, coeffs=None) -> CeremonyResult:
        """g16_params_check_delta: `after` is `before` with more delta multiplied in (any number of contribute_delta calls): the part
        no contribution touches is byte-equal, delta_g1 / delta_g2 moved by one ratio, and l_query / h_query by its inverse.  Who
        contributed is not attested -- only that the chain of ratios holds.  ValueError for keys of different shapes."""
        _host_key(before, "check_delta_contribution")
        _host_key(after, "check_delta_contribution")
        b, a, (nv, ni, nl, nh) = _delta_check_args(self.curve, before, after)
        co, cp, nco = _coeff_args(coeffs)
        info = CeremonyInfoC()
        bv, av = _params_view(b), _params_view(a)
        lb = self._ctx.lib
        lb.check(lb.cer.g16_params_check_delta(self._ctx.handle, C.byref(bv), C.byref(av), nv, ni, nl, nh, cp, nco, C.byref(info)))
        return CeremonyResult.from_info(info, KEY_CHECK_FLAGS, KEY_POINT_ARRAYS, KEY_FIXED_ARRAYS)

    def check_parameters(self, matrices: ConstraintMatrices, srs: SRS, pk: ProvingKey, coeffs=None, derive: bool = True) -> CeremonyResult:
        """What snarkjs calls `zkey verify`: check_srs, then the delta = 1 key of (matrices, srs) by generate_parameters_from_srs, then
        check_delta_contribution(derived, pk).  Returns the first result that fails, else the passing key result.
        derive=False decides the same question without deriving the key: check_srs, then check_key_derivation (whose flags and
        arrays the result then carries)."""
        res = self.check_srs(srs, coeffs)
        if not res:
            return res
        if not derive:
            return self.check_key_derivation(matrices, srs, pk, coeffs)
        derived = self.generate_parameters_from_srs(matrices, srs)
        return self.check_delta_contribution(derived, pk, coeffs)

    # -- the key check without the derivation: the SRS folded under the circuit's matrices ----------------------------
    def check_key_derivation(self, matrices: ConstraintMatrices, srs: SRS, pk: ProvingKey, coeffs=None) -> CeremonyResult:
        """g16_params_check_derivation: `pk` is the key of (matrices, srs) for this object's reduction, after any number of delta
        contributions -- decided by random linear combinations pushed through the matrices and the scalar transform onto the SRS
        (a sparse mat-vec, seven scalar transforms, MSMs over the raw SRS points: no transform over the group).  PRECONDITION: the
        SRS passes check_srs (check_parameters(derive=False) runs it first).  coeffs: 128-bit coefficients as in check_srs, at
        least max(variables, len(h_query)) of them, fixed AFTER the key; None draws fresh ones.  With the key's points in their
        subgroups (BAD_POINT otherwise) a key that differs from the true one in any point passes with probability <= 2^-128.
        ValueError for a key of another shape; not attested: who contributed, gamma != 1."""
        _host_key(pk, "check_key_derivation")
        ni, nc, nv = _derivation_shape(self.curve, matrices, srs)
        key = _derivation_key(self.curve, self.qap, matrices, pk)
        views, keep = _csr_views(matrices)
        sv, skeep = srs.view()
        kv = _params_view(key)
        co, cp, nco = _coeff_args(coeffs)
        info = CeremonyInfoC()
        lb = self._ctx.lib
        lb.check(lb.kc.g16_params_check_derivation(self._ctx.handle, views, ni, nc, nv, self.qap.QAP_ID, C.byref(sv), C.byref(kv), cp, nco,
                                                   C.byref(info)))
        return CeremonyResult.from_info(info, KEY_DERIVATION_FLAGS, KEY_DERIVATION_ARRAYS, KEY_DERIVATION_FIXED)

    def fold_key_from_srs(self, matrices: ConstraintMatrices, srs: SRS, coeffs) -> Dict[str, np.ndarray]:
        """g16_key_fold_from_srs: the SRS side of check_key_derivation's equations A, B_G1, B_G2, GAMMA_ABC, L, H before any pairing --
        a dict of six affine points (keys a, b_g1, b_g2, gamma_abc, l, h).  For the true key these are sum rho_j (query point j)
        with delta = 1.  Deterministic: coeffs are required."""
        ni, nc, nv = _derivation_shape(self.curve, matrices, srs)
        views, keep = _csr_views(matrices)
        sv, skeep = srs.view()
        co, cp, nco = _fold_coeffs(coeffs)
        pts, out = _fold_out(self.curve)
        lb = self._ctx.lib
        lb.check(lb.kc.g16_key_fold_from_srs(self._ctx.handle, views, ni, nc, nv, self.qap.QAP_ID, C.byref(sv), cp, nco, C.byref(out)))
        return pts

    def keycheck_timings(self) -> dict:
        """g16_keycheck_get_timings: milliseconds of the last check_key_derivation / fold_key_from_srs on this object (upload,
        membership, rows, transforms, sorts, passes, reductions by stream events; pairings on the wall clock) and the plan of the
        full-size scalar sorts over the raw SRS bases (window_bits, windows)"""
        tm = KeycheckTimingsC()
        self._ctx.lib.check(self._ctx.lib.kc.g16_keycheck_get_timings(self._ctx.handle, C.byref(tm)))
        return tm.as_dict()

    def ceremony_timings(self) -> dict:
        """g16_ceremony_get_timings: milliseconds of the last rlc_sums / check_srs / check_delta_contribution on this object (upload,
        membership, sort, passes, reductions by stream events; pairings on the wall clock)"""
        tm = CeremonyTimingsC()
        self._ctx.lib.check(self._ctx.lib.cer.g16_ceremony_get_timings(self._ctx.handle, C.byref(tm)))
        return tm.as_dict()

    # -- phase 1: one scalar per point, a contribution to the powers of tau, its check ------------------------------
    def batch_scalar_mul(self, points: np.ndarray, scalars: np.ndarray) -> np.ndarray:
        """g16_batch_scalar_mul: out[i] = scalars[i] * points[i] over n affine points of G1 or G2 (told apart by the row width) and n
        scalars (Fr, Montgomery limbs).  Exact for every scalar and every point with coordinates below the modulus, in the subgroup
        or not; no membership test is made."""
        pts, sc, g2, out = _smul_args(self.curve, points, scalars)
        lb = self._ctx.lib
        lb.check(lb.ph1.g16_batch_scalar_mul(self._ctx.handle, g2, ptr64(pts.reshape(-1)), ptr64(sc.reshape(-1)), len(pts), ptr64(out.reshape(-1))))
        return out

    def contribute_tau(self, srs: SRS, tau=None, alpha=None, beta=None) -> Tuple[SRS, "TauContribution"]:
        """g16_srs_contribute on a copy of the SRS: tau_g1[i], tau_g2[i] <- tau^i (.), alpha_tau_g1[i] <- alpha tau^i (.),
        beta_tau_g1[i] <- beta tau^i (.), beta_g2 <- beta (.); the contributor's public record comes back beside the new SRS.  `srs`
        itself is untouched.  A secret left None is drawn from the operating system, non-zero, and is not returned.
        UnexpectedIdentity for a zero secret."""
        sec, new, pub = _contribution_setup(self.curve, srs, tau, alpha, beta)
        sv, keep = new.view()
        pv, pkeep = pub.view()
        lb = self._ctx.lib
        lb.check(lb.ph1.g16_srs_contribute(self._ctx.handle, ptr64(sec[0]), ptr64(sec[1]), ptr64(sec[2]), C.byref(sv), C.byref(pv), None))
        return new, pub

    def check_tau_contribution(self, before: SRS, after: SRS, contribution: "TauContribution", coeffs=None) -> CeremonyResult:
        """g16_srs_check_contribution: `after` passes check_srs and descends from `before` by the contribution whose G2 images are
        `contribution` -- the generators and lengths unchanged (SHAPE), tau_g1[1], alpha_tau_g1[0] and beta_tau_g1[0] moved by the
        ratios the record holds (TAU_RATIO, ALPHA_RATIO, BETA_RATIO).  `before` is read at five points only.  Who contributed is not
        attested.  coeffs: as check_srs."""
        bv, av, pv, keep = _tau_check_args(self.curve, before, after, contribution)
        co, cp, nco = _coeff_args(coeffs)
        info = CeremonyInfoC()
        lb = self._ctx.lib
        lb.check(lb.ph1.g16_srs_check_contribution(self._ctx.handle, C.byref(bv), C.byref(av), C.byref(pv), cp, nco, C.byref(info)))
        return CeremonyResult.from_info(info, TAU_CHECK_FLAGS, TAU_ARRAYS)

    def phase1_timings(self) -> dict:
        """g16_phase1_get_timings: stream-event milliseconds of the last batch_scalar_mul / contribute_tau on this object (upload,
        powers, multiplications G1, multiplications G2, download), summed over the chunks"""
        tm = Phase1TimingsC()
        self._ctx.lib.check(self._ctx.lib.ph1.g16_phase1_get_timings(self._ctx.handle, C.byref(tm)))
        return tm.as_dict()

    def srs_timings(self) -> dict:
        """g16_srs_get_timings: stream-event milliseconds of the last generate_parameters_from_srs (transforms, products, h) and
        contribute_delta (delta) on this object"""
        tm = SrsTimingsC()
        self._ctx.lib.check(self._ctx.lib.c.g16_srs_get_timings(self._ctx.handle, C.byref(tm)))
        return tm.as_dict()

    # -- generator.rs:20-45 (+ lib.rs:63-74 circuit_specific_setup) -------------------------------
    def generate_random_parameters_with_reduction(self, circuit, rng=None) -> ProvingKey:
        """Groth16::generate_random_parameters_with_reduction: synthesise `circuit` in setup mode on the host, draw the toxic
        waste, random generators (a random multiple of the curve's standard generator, as E::G1::rand does up to distribution)
        and t outside the domain from `rng`, and build the key on the GPU (generate_parameters_with_qap)."""
        from .r1cs import synthesize

        cs = synthesize(self.curve, circuit, setup_mode=True)
        matrices = cs.to_matrices()
        lb = self._ctx.lib
        g1s, g2s = _GENERATORS[self.curve]
        L = FQ_LIMBS[self.curve]

        def rand_generator(g2: bool) -> np.ndarray:
            k = _rand_fr(self.curve, rng, nonzero=True)   # read as a plain integer below r: any non-zero multiple will do
            base = _fq_mont(self.curve, [g2s[0][0], g2s[0][1], g2s[1][0], g2s[1][1]] if g2 else list(g1s))
            out = np.zeros((4 if g2 else 2) * L, dtype=np.uint64)
            lb.check(lb.c.g16_host_group_op(CURVE_ID[self.curve], int(g2), 1, ptr64(base), ptr64(k), ptr64(out)))
            return out

        need, n = matrices.num_constraints + matrices.num_instance_variables, 1
        while n < need:
            n <<= 1
        p = _MODULUS_R[self.curve]
        rinv = pow(1 << 256, -1, p)
        while True:   # domain.sample_element_outside_domain(rng), generator.rs:90
            t = _rand_fr(self.curve, rng, nonzero=True)
            tv = int.from_bytes(t.tobytes(), "little") * rinv % p
            if pow(tv, n, p) != 1 and (self.qap.QAP_ID == QAP_LIBSNARK or pow(tv, 2 * n, p) != 1):   # Circom: nor t = rho^odd
                break
        alpha, beta, gamma, delta = (_rand_fr(self.curve, rng, nonzero=True) for _ in range(4))
        return self.generate_parameters_with_qap(matrices, alpha, beta, gamma, delta, rand_generator(False), rand_generator(True), t)

    def setup(self, circuit, rng=None) -> Tuple[ProvingKey, ProvingKey]:
        """SNARK::circuit_specific_setup (lib.rs:63-74): (pk, vk); the vk is the key's own alpha_g1 / beta_g2 / gamma_g2 / delta_g2
        / gamma_abc_g1 fields (data_structures.rs:28-41), returned as the same object"""
        pk = self.generate_random_parameters_with_reduction(circuit, rng)
        return pk, pk

    # -- prover.rs:173-217 ------------------------------------------------------------------------
    _MAX_CIRCUITS_BY_CONTENT = 64

    def create_proof_with_reduction(self, circuit, pk: ProvingKey, r: np.ndarray, s: np.ndarray, circuit_id=None, check: bool = False) -> Proof:
        """(check: see create_proof_with_reduction_and_matrices.)  Groth16::create_proof_with_reduction: host-side synthesis exactly as prover.rs:185-204 (fresh constraint system,
        generate_constraints, matrices, full_assignment = instance ++ witness), then the pure-data call on the GPU.  The
        device copy of the matrices is cached, so proving the same circuit again uploads only the assignment: by
        `circuit_id` (any hashable the caller vouches for: same id = same constraint matrices; no hashing at all) or, without
        one, by a SHA-1 of the matrices' content (bounded: the oldest entry and its device copy are dropped past 64 circuits --
        which also invalidates any DistributedWitnessMap still holding that circuit's handle: create those after the circuits)."""
        import hashlib

        from .r1cs import synthesize

        cs = synthesize(self.curve, circuit, setup_mode=False)
        m = cs.to_matrices()
        if circuit_id is not None:
            key = ("id", circuit_id)
        else:
            h = hashlib.sha1()
            for mat in (m.a, m.b, m.c):
                for arr in mat:
                    h.update(np.ascontiguousarray(arr).tobytes())
            h.update(repr((m.num_instance_variables, m.num_witness_variables, m.num_constraints)).encode())
            key = h.digest()
        known = self._circuits_by_content.get(key)
        if known is None:
            if len(self._circuits_by_content) >= self._MAX_CIRCUITS_BY_CONTENT:
                old_key = next(iter(self._circuits_by_content))
                old = self._circuits_by_content.pop(old_key)
                ent = self._cks.pop(id(old), None)
                if ent is not None:
                    ent[1].close()
            self._circuits_by_content[key] = m
        else:
            if circuit_id is not None:
                # the caller vouches that one id means one circuit; the cheap invariants are checked anyway -- a reused id would
                # otherwise prove against the WRONG device matrices and hand back an invalid proof without any error
                def shape(mm):
                    return (mm.num_instance_variables, mm.num_witness_variables, mm.num_constraints,
                            tuple(int(np.asarray(mat[0])[-1]) for mat in (mm.a, mm.b, mm.c)))   # row_ptr[-1] = nnz of A, B, C

                if shape(known) != shape(m):
                    raise ValueError(f"circuit_id {circuit_id!r} was first used for a circuit of shape {shape(known)} (instance, witness, "
                                     f"constraints, nnz) and is now passed with one of shape {shape(m)}: one id must mean one circuit")
            m = known
        return self.create_proof_with_reduction_and_matrices(pk, r, s, m, cs.num_instance_variables, cs.num_constraints, cs.full_assignment(),
                                                             check=check)

    def prove(self, pk: ProvingKey, circuit, rng=None, check: bool = False) -> Proof:
        """SNARK::prove (lib.rs:76-82) = create_random_proof_with_reduction(circuit, pk, rng) (prover.rs:138-150)"""
        return self.create_proof_with_reduction(circuit, pk, _rand_fr(self.curve, rng), _rand_fr(self.curve, rng), check=check)

    def create_proof_no_zk(self, circuit, pk: ProvingKey, check: bool = False) -> Proof:
        """prover.rs:155-168 on a circuit: r = s = 0 (same as create_proof_with_reduction_no_zk(circuit, pk))"""
        zero = np.zeros(4, dtype=np.uint64)
        return self.create_proof_with_reduction(circuit, pk, zero, zero, check=check)

    # -- verifier.rs:13-76, lib.rs:84-96 ----------------------------------------------------------
    def prepare_verifying_key(self, vk) -> "PreparedVerifyingKey":
        """verifier.rs:13-20: e(alpha, beta), -gamma / -delta prepared and gamma_abc_g1's window tables, resident on this object's
        GPU(s).  `vk`: a VerifyingKey or a ProvingKey that carries gamma_g2 / gamma_abc_g1."""
        from .verifier import PreparedVerifyingKey
        return PreparedVerifyingKey(self._ctx, vk)

    def process_vk(self, vk) -> "PreparedVerifyingKey":   # lib.rs:84-86
        return self.prepare_verifying_key(vk)

    def prepare_inputs(self, pvk, public_inputs) -> np.ndarray:
        """verifier.rs:25-39 (host): gamma_abc_g1[0] + sum x_i gamma_abc_g1[i + 1] as G1 affine; MalformedVerifyingKey on a length
        mismatch"""
        from .binding import MalformedVerifyingKey
        from .verifier import as_vk
        vk = as_vk(pvk.vk if hasattr(pvk, "vk") else pvk)
        L = FQ_LIMBS[self.curve]
        x = [_c(v).reshape(4) for v in public_inputs] if len(public_inputs) else []
        bases = _c(vk.gamma_abc_g1).reshape(-1, 2 * L)
        if len(x) + 1 != bases.shape[0]:
            raise MalformedVerifyingKey(11, "malformed verifying key: public inputs + 1 != gamma_abc_g1")
        lb, cid = self._ctx.lib, CURVE_ID[self.curve]
        acc = bases[0].copy()
        for xi, b in zip(x, bases[1:]):
            k, t, s = np.zeros(4, dtype=np.uint64), np.zeros(2 * L, dtype=np.uint64), np.zeros(2 * L, dtype=np.uint64)
            lb.check(lb.c.g16_host_field_op(cid, 0, 4, ptr64(_c(xi)), None, ptr64(k)))          # canonical x_i
            lb.check(lb.c.g16_host_group_op(cid, 0, 1, ptr64(_c(b)), ptr64(k), ptr64(t)))       # x_i * base
            lb.check(lb.c.g16_host_group_op(cid, 0, 0, ptr64(acc), ptr64(t), ptr64(s)))         # acc + that
            acc = s
        return acc

    def verify_proof_with_prepared_inputs(self, pvk, proof: Proof, prepared_inputs: np.ndarray) -> bool:   # verifier.rs:44-65
        from .verifier import verify_batch_prepared
        return bool(verify_batch_prepared(self._ctx, pvk, [proof], _c(prepared_inputs).reshape(1, -1))[0] == 1)

    def verify_proof(self, pvk, proof: Proof, public_inputs) -> bool:   # verifier.rs:68-76
        return bool(self.verify_proofs(pvk, [proof], [public_inputs])[0])

    def verify_with_processed_vk(self, pvk, x, proof: Proof) -> bool:   # lib.rs:88-96
        return self.verify_proof(pvk, proof, x)

    def verify_proofs(self, pvk, proofs: Sequence[Proof], public_inputs_list) -> np.ndarray:
        """verify_proof over a batch, one GPU lane per proof: a bool per proof"""
        return self.verify_verdicts(pvk, proofs, public_inputs_list) == 1

    def verify_verdicts(self, pvk, proofs, public_inputs_list) -> np.ndarray:
        """g16_verify_batch's verdict bytes: 1 accept, 0 reject, 2 a point of the proof is off its curve"""
        from .verifier import verify_batch
        return verify_batch(self._ctx, pvk, proofs, public_inputs_list)

    def verify_aggregate_verdict(self, pvk, proofs, public_inputs_list, coeffs=None, check_subgroups: bool = False) -> int:
        """g16_verify_aggregate: the whole batch in one randomised equation with one final exponentiation.  1 every proof is
        accepted, 0 at least one is not, 2 a point is off its curve.  coeffs: one non-zero 128-bit integer per proof, fixed after
        the proofs; None draws them from the operating system.  Sound for proofs whose points are in the prime-order subgroups:
        check_subgroups=True (g16_verify_aggregate_checked) tests that on the GPU before the equation and is the call whose
        contract needs no such proviso -- it answers 3 when every point is on its curve but one is outside its subgroup (2 wins
        over 3, 3 over 0 / 1).  With the default False the caller vouches for the points (proof_from_bytes(validate=2) checks
        them on the host)."""
        from .verifier import verify_aggregate
        return verify_aggregate(self._ctx, pvk, proofs, public_inputs_list, coeffs, check_subgroups)

    def verify_proofs_aggregate(self, pvk, proofs, public_inputs_list, coeffs=None, check_subgroups: bool = False) -> bool:
        return self.verify_aggregate_verdict(pvk, proofs, public_inputs_list, coeffs, check_subgroups) == 1

    def verify_proofs_aggregate_or_each(self, pvk, proofs, public_inputs_list, check_subgroups: bool = False) -> np.ndarray:
        """a bool per proof: the aggregate check first, and only if it fails verify_proofs to name the culprits.  With
        check_subgroups=True a proof with a point outside its subgroup (or off its curve) is answered False and the per-proof
        verifier runs on the rest"""
        verdict = self.verify_aggregate_verdict(pvk, proofs, public_inputs_list, check_subgroups=check_subgroups)
        n = len(public_inputs_list)
        if verdict == 1:
            return np.ones(n, dtype=bool)
        if not check_subgroups:
            return self.verify_proofs(pvk, proofs, public_inputs_list)
        from .verifier import _flat_proofs
        flat = _flat_proofs(proofs, self.curve)
        keep = np.flatnonzero(self.check_proof_subgroups(flat) == 1)
        out = np.zeros(n, dtype=bool)
        if keep.size:
            out[keep] = self.verify_proofs(pvk, flat[keep], [public_inputs_list[i] for i in keep])
        return out

    def verify_aggregate_mixed_verdict(self, pvks, key_of, proofs, public_inputs_list, coeffs=None, check_subgroups: bool = False) -> int:
        """g16_verify_aggregate_mixed: a batch whose proofs were made under several keys (proof i under pvks[key_of[i]], in any
        order) in ONE randomised equation with one final exponentiation; the per-key pairs run on the GPU, one lane per key.
        public_inputs_list[i] holds as many inputs as proof i's key takes.  Verdicts, coeffs and check_subgroups as
        verify_aggregate_verdict.  A multi-device prover runs the call on its first device"""
        from .verifier import verify_aggregate_mixed
        return verify_aggregate_mixed(self._ctx, pvks, key_of, proofs, public_inputs_list, coeffs, check_subgroups)

    def verify_proofs_aggregate_mixed(self, pvks, key_of, proofs, public_inputs_list, coeffs=None, check_subgroups: bool = False) -> bool:
        return self.verify_aggregate_mixed_verdict(pvks, key_of, proofs, public_inputs_list, coeffs, check_subgroups) == 1

    def verify_proofs_aggregate_mixed_or_each(self, pvks, key_of, proofs, public_inputs_list, check_subgroups: bool = False) -> np.ndarray:
        """a bool per proof, in input order: the mixed aggregate check first, and only if it fails verify_verdicts once per key to
        name the culprits.  With check_subgroups=True a proof with a point outside its subgroup (or off its curve) is answered
        False"""
        verdict = self.verify_aggregate_mixed_verdict(pvks, key_of, proofs, public_inputs_list, check_subgroups=check_subgroups)
        n = len(public_inputs_list)
        if verdict == 1:
            return np.ones(n, dtype=bool)
        from .verifier import _flat_proofs
        flat = _flat_proofs(proofs, self.curve)
        ko = np.asarray(key_of, dtype=np.int64).reshape(-1)
        ok = self.check_proof_subgroups(flat) == 1 if check_subgroups else np.ones(n, dtype=bool)
        out = np.zeros(n, dtype=bool)
        for k in np.unique(ko):
            idx = np.flatnonzero((ko == k) & ok)
            if idx.size:
                out[idx] = self.verify_verdicts(pvks[k], flat[idx], [public_inputs_list[i] for i in idx]) == 1
        return out

    def check_subgroups(self, points, g2: bool = False) -> np.ndarray:
        """prime-order subgroup membership of affine points on the GPU (g16_check_subgroups): a uint8 per point -- 1 in the
        subgroup, 0 on the curve but outside it, 2 off the curve"""
        from .verifier import check_subgroups
        return check_subgroups(self._ctx, points, g2)

    def decompress_points(self, data, g2: bool = False):
        """compressed points (bytes or a uint8 array; G2 with g2=True) decoded on the GPU (g16_decompress_points) by the rules of
        deserialize_points(compressed=True, validate=0): (points, status), status 1 decoded / 0 an invalid encoding, whose point
        is the identity.  ValueError for a length that is no multiple of the encoding size"""
        from .verifier import decompress_points
        return decompress_points(self._ctx, data, g2)

    def decode_points(self, data, g2: bool = False, compressed: bool = True, validate: int = 2):
        """encoded points of either form decoded AND validated on the GPU (g16_decode_points), point by point what
        deserialize_points(compressed, validate) does to each: (points, status), status 1 and the point where that call accepts
        it, else the identity and 0 the bytes do not decode / 2 off the curve / 3 outside the prime-order subgroup"""
        from .verifier import decode_points
        return decode_points(self._ctx, data, g2, compressed, validate)

    def decode_points_host(self, data, g2: bool = False, compressed: bool = True, validate: int = 2):
        """decode_points by the same templates on the CPU (g16_host_decode_points)"""
        from .verifier import decode_points_host
        return decode_points_host(self.curve, data, g2, compressed, validate)

    def load_proving_key_bytes(self, data, compressed: bool = True, validate: int = 2) -> DeviceProvingKey:
        """a serialized ProvingKey (proving_key_to_bytes' form) onto this object's GPU without the detour through host arrays
        (g16_pk_load_bytes): the five queries are uploaded as bytes, decoded and validated on the device and turned into the
        prover's window tables there.  validate as proving_key_from_bytes.  A key that call would refuse raises InvalidData
        naming the first failing point in file order (.section, .index, .reason, .n_bad); nothing stays allocated.  Single-device
        objects only."""
        from .serialize import _Reader
        if self._owner is not None:
            raise ValueError("keys are loaded through the object that owns the device data (share_device_data_of)")
        buf = bytes(data)   # (no copy of a bytes object)
        info, handle, lb = PkBytesInfoC(), C.c_void_p(), self._ctx.lib
        lb.check(lb.c.g16_pk_load_bytes(self._ctx.handle, buf, len(buf), int(bool(compressed)), int(validate), C.byref(handle), C.byref(info),
                                        C.sizeof(info)), pk_bytes_info=info)
        dpk = _DevicePk.from_handle(self._ctx, handle)
        r = _Reader(self.curve, buf, compressed, 0)   # the head again, for the host (already validated by the call above)
        head = dict(alpha_g1=r.point(False), beta_g2=r.point(True), gamma_g2=r.point(True), delta_g2=r.point(True), gamma_abc_g1=r.vec(False),
                    beta_g1=r.point(False), delta_g1=r.point(False))
        key = DeviceProvingKey(self.curve, head, info.counts(), int(info.consumed), self._ctx, dpk)
        self._byte_keys.append(key)
        return key

    def decompress_proofs(self, data):
        """compressed proofs A | B | C (proof_to_bytes(compressed=True), concatenated) decoded on the GPU (g16_decompress_proofs):
        (flat_proofs, status) -- the array verify_proofs takes and a byte per proof, 1 iff its three points decode"""
        from .verifier import decompress_proofs
        return decompress_proofs(self._ctx, data)

    def verify_aggregate_bytes_verdict(self, pvk, data, public_inputs_list, coeffs=None) -> int:
        """bytes to verdict (g16_verify_aggregate_bytes): the compressed proofs are uploaded, decoded, membership-tested and put
        through the aggregate equation on the GPU without returning to the host.  1 / 0 / 3 as
        verify_aggregate_verdict(check_subgroups=True), 4: some proof's bytes do not decode (decompress_proofs names it; 4 wins
        over 3)"""
        from .verifier import verify_aggregate_bytes
        return verify_aggregate_bytes(self._ctx, pvk, data, public_inputs_list, coeffs)

    def verify_proofs_aggregate_bytes(self, pvk, data, public_inputs_list, coeffs=None) -> bool:
        return self.verify_aggregate_bytes_verdict(pvk, data, public_inputs_list, coeffs) == 1

    def check_proof_subgroups(self, proofs) -> np.ndarray:
        """the same per proof (g16_check_proof_subgroups): 2 if A, B or C is off its curve, otherwise 0 if one is outside its
        subgroup, otherwise 1"""
        from .verifier import check_proof_subgroups
        return check_proof_subgroups(self._ctx, proofs)

    def pairing(self, g1s: np.ndarray, g2s: np.ndarray) -> np.ndarray:
        """prod e(g1s[i], g2s[i]) on the GPU (GT as arkworks' 12 Fq limbs)"""
        from .verifier import device_pairing
        return device_pairing(self._ctx, g1s, g2s)

    # -- prover.rs:223-250 ----------------------------------------------------------------------
    def rerandomize_proof(self, vk: ProvingKey, proof: Proof, rng=None) -> Proof:
        return rerandomize_proof(self.curve, vk, proof, rng)

    # -- prover.rs:26-51 -------------------------------------------------------------------
    def create_proof_with_reduction_and_matrices(self, pk: ProvingKey, r: np.ndarray, s: np.ndarray, matrices: ConstraintMatrices,
                                                 num_inputs: int, num_constraints: int, full_assignment: np.ndarray, check: bool = False) -> Proof:
        """check=False is the reference's release build: the assignment is proved as given, and one that does not satisfy the
        constraints yields a well-formed proof no verifier accepts.  check=True keeps debug_assert!(cs.is_satisfied()) of
        prover.rs:193 (g16_prove_checked): the assignment is checked on the GPU first and `Unsatisfiable` -- with the first failing
        row and its values -- is raised instead of proving; a satisfied one gives the same proof bit for bit."""
        assert num_inputs == matrices.num_instance_variables and num_constraints == matrices.num_constraints
        L = FQ_LIMBS[self.curve]
        dpk, dck = self._pk(pk, num_inputs), self._ck(matrices, for_check=check)
        z = _c(full_assignment)
        out = ProofC()
        lb = self._ctx.lib
        if check:
            res = CheckResultC()
            lb.check(lb.c.g16_prove_checked(self._ctx.handle, dpk.handle, dck.handle, z.ctypes.data, z.shape[0], 0, ptr64(_c(r)), ptr64(_c(s)),
                                            C.byref(out), C.byref(res)), res)
        else:
            lb.check(lb.c.g16_prove(self._ctx.handle, dpk.handle, dck.handle, z.ctypes.data, z.shape[0], 0, ptr64(_c(r)), ptr64(_c(s)),
                                    C.byref(out)))
        return Proof(np.array(out.a[: 2 * L], dtype=np.uint64), np.array(out.b[: 4 * L], dtype=np.uint64),
                     np.array(out.c[: 2 * L], dtype=np.uint64))

    # -- prover.rs:193: cs.is_satisfied() / cs.which_is_unsatisfied() (ark-relations) on the GPU ------------------------------
    def check_assignment(self, matrices: ConstraintMatrices, full_assignment: Optional[np.ndarray], z_dev_ptr: int = 0) -> CheckResult:
        """g16_circuit_check: how many constraint rows `full_assignment` fails, the first of them and its three sums.  z_dev_ptr != 0:
        the assignment is read from device memory in place (`full_assignment` is then not looked at).  With CircomReduction the C
        matrix, which the map never reads, is uploaded on the first check of a circuit."""
        dck = self._ck(matrices, for_check=True)
        res = CheckResultC()
        lb = self._ctx.lib
        if z_dev_ptr:
            lb.check(lb.c.g16_circuit_check(self._ctx.handle, dck.handle, C.c_void_p(z_dev_ptr), dck.num_variables, 1, C.byref(res)))
        else:
            z = _c(full_assignment)
            lb.check(lb.c.g16_circuit_check(self._ctx.handle, dck.handle, z.ctypes.data, z.shape[0], 0, C.byref(res)))
        return CheckResult.from_c(res)

    def is_satisfied(self, matrices: ConstraintMatrices, z: np.ndarray) -> bool:
        """cs.is_satisfied()"""
        return self.check_assignment(matrices, z).satisfied

    def which_is_unsatisfied(self, matrices: ConstraintMatrices, z: np.ndarray) -> Optional[int]:
        """cs.which_is_unsatisfied(): the index of the first failing row (the reference names it by its trace), None if none"""
        return self.check_assignment(matrices, z).first_row

    # -- prover.rs:155-168 -----------------------------------------------------------------
    def create_proof_with_reduction_no_zk(self, *args) -> Proof:
        """the reference's signature ``(circuit, pk)`` (prover.rs:155-168), or the pure-data form
        ``(pk, matrices, num_inputs, num_constraints, full_assignment)``: r = s = 0"""
        zero = np.zeros(4, dtype=np.uint64)
        if len(args) == 2 and not isinstance(args[0], (ProvingKey, DeviceProvingKey)):
            return self.create_proof_with_reduction(args[0], args[1], zero, zero)
        pk, matrices, num_inputs, num_constraints, full_assignment = args
        return self.create_proof_with_reduction_and_matrices(pk, zero, zero, matrices, num_inputs, num_constraints, full_assignment)

    # -- prover.rs:138-150 -----------------------------------------------------------------
    def create_random_proof_with_reduction(self, *args, rng=None) -> Proof:
        """the reference's signature ``(circuit, pk, rng)`` (prover.rs:138-150), or the pure-data form
        ``(pk, matrices, num_inputs, num_constraints, full_assignment[, rng])``: fresh r, s from rng"""
        if not isinstance(args[0], (ProvingKey, DeviceProvingKey)):
            circuit, pk = args[0], args[1]
            rng = args[2] if len(args) > 2 else rng
            return self.create_proof_with_reduction(circuit, pk, _rand_fr(self.curve, rng), _rand_fr(self.curve, rng))
        pk, matrices, num_inputs, num_constraints, full_assignment = args[:5]
        rng = args[5] if len(args) > 5 else rng
        return self.create_proof_with_reduction_and_matrices(pk, _rand_fr(self.curve, rng), _rand_fr(self.curve, rng), matrices, num_inputs,
                                                             num_constraints, full_assignment)

    # -- r1cs_to_qap.rs:172-235 (QAP::witness_map_from_matrices: this object's reduction) -------
    def witness_map_from_matrices(self, matrices: ConstraintMatrices, num_inputs: int, num_constraints: int,
                                  full_assignment: np.ndarray) -> np.ndarray:
        dck = self._ck(matrices)
        z = _c(full_assignment)
        h = np.zeros((dck.domain_size, 4), dtype=np.uint64)
        lb = self._ctx.lib
        lb.check(lb.c.g16_witness_map(self._ctx.handle, dck.handle, z.ctypes.data, z.shape[0], 0, ptr64(h)))
        return h

    # -- VariableBaseMSM::msm (scalars in Montgomery form; into_bigint happens on the GPU) ----
    def msm(self, bases: np.ndarray, scalars: np.ndarray, g2: bool = False) -> np.ndarray:
        L = FQ_LIMBS[self.curve]
        n = min(len(bases), len(scalars))  # msm_bigint truncates to the shorter input
        b, s = _c(bases[:n]), _c(scalars[:n])
        out = np.zeros((4 if g2 else 2) * L, dtype=np.uint64)
        lb = self._ctx.lib
        fn = lb.c.g16_msm_g2 if g2 else lb.c.g16_msm_g1
        lb.check(fn(self._ctx.handle, ptr64(b) if n else None, ptr64(s) if n else None, n, ptr64(out)))
        return out

    def msm_bucket_shard(self, bases: np.ndarray, scalars: np.ndarray, rank: int, world: int, g2: bool = False) -> np.ndarray:
        """g16_msm_bucket_shard: rank's bucket-space share of msm(bases, scalars) -- the `world` results add up to the MSM"""
        L = FQ_LIMBS[self.curve]
        n = min(len(bases), len(scalars))
        b, s = _c(bases[:n]), _c(scalars[:n])
        out = np.zeros((4 if g2 else 2) * L, dtype=np.uint64)
        lb = self._ctx.lib
        lb.check(lb.c.g16_msm_bucket_shard(self._ctx.handle, int(g2), ptr64(b) if n else None, ptr64(s) if n else None, n, rank, world, ptr64(out)))
        return out

    # -- EvaluationDomain::{fft, ifft, coset variants}, natural order ---------------------------
    def ntt(self, data: np.ndarray, inverse: bool = False, coset: bool = False) -> np.ndarray:
        d = _c(data).copy()
        n = d.shape[0]
        log_n = n.bit_length() - 1
        if 1 << log_n != n:
            raise ValueError("length must be a power of two")
        lb = self._ctx.lib
        lb.check(lb.c.g16_ntt(self._ctx.handle, ptr64(d), log_n, int(inverse), int(coset)))
        return d

    def pk_info(self, pk: ProvingKey, num_inputs: int, shard=(0, 1), dist_h: bool = False) -> dict:
        """how the device-resident copy of (this shard of) the key is held: g16_pk_get_info"""
        return self._pk(pk, num_inputs, shard, dist_h).info()

    def timings(self) -> dict:
        t = TimingsC()
        self._ctx.lib.check(self._ctx.lib.c.g16_get_timings(self._ctx.handle, C.byref(t)))
        return t.as_dict()

    # -- sharded form --------------------------------------------------------------------------
    def prove_partial(self, pk: ProvingKey, matrices: ConstraintMatrices, full_assignment: np.ndarray, shard: Tuple[int, int],
                      skip_b_g1: bool = False) -> bytes:
        _host_key(pk, "prove_partial")
        dpk, dck = self._pk(pk, matrices.num_instance_variables, shard), self._ck(matrices)
        z = _c(full_assignment)
        part = PartialC()
        lb = self._ctx.lib
        lb.check(lb.c.g16_prove_partial(self._ctx.handle, dpk.handle, dck.handle, z.ctypes.data, z.shape[0], 0, int(skip_b_g1),
                                        C.byref(part)))
        return bytes(part)

    def prove_partial_prepare(self, pk: ProvingKey, matrices: ConstraintMatrices, z_dev_ptr: int, n_assign: int, shard: Tuple[int, int],
                              dist_h: bool = True):
        """g16_prove_partial_prepare: enqueue the witness digit/sort pass of the next prove_partial[_h] over this key shard and this
        DEVICE assignment now -- before the distributed witness map's stages -- so that the two run side by side"""
        _host_key(pk, "prove_partial_prepare")
        dpk, dck = self._pk(pk, matrices.num_instance_variables, shard, dist_h=dist_h), self._ck(matrices)
        lb = self._ctx.lib
        lb.check(lb.c.g16_prove_partial_prepare(self._ctx.handle, dpk.handle, dck.handle, C.c_void_p(z_dev_ptr), n_assign))

    def prove_finalize_prepare(self, pk: ProvingKey, num_inputs: int, r: np.ndarray, s: np.ndarray, shard: Tuple[int, int],
                               dist_h: bool = False):
        """g16_prove_finalize_prepare: start the (r, s)-only half of the glue of prover.rs:76-131 on a host thread now, so that it
        runs while the GPU computes this rank's partial sums; the next `finalize` over the same (key shard, r, s) picks it up"""
        _host_key(pk, "prove_finalize_prepare")
        dpk = self._pk(pk, num_inputs, shard, dist_h=dist_h)
        lb = self._ctx.lib
        lb.check(lb.c.g16_prove_finalize_prepare(self._ctx.handle, dpk.handle, ptr64(np.ascontiguousarray(r, dtype=np.uint64)),
                                                 ptr64(np.ascontiguousarray(s, dtype=np.uint64))))

    def prove_partial_h(self, pk: ProvingKey, matrices: ConstraintMatrices, full_assignment, shard: Tuple[int, int],
                        h_dev_ptr: int, h_len: int, skip_b_g1: bool = False, z_dev_ptr: int = 0) -> bytes:
        """g16_prove_partial_h: the shard's five partial sums with h supplied by the caller (device memory: this rank's block of
        the distributed witness map); the key shard is the one gathered in that block order (dist_h).  z_dev_ptr != 0: the
        assignment is taken from device memory (`full_assignment` then only gives the length)"""
        _host_key(pk, "prove_partial_h")
        dpk, dck = self._pk(pk, matrices.num_instance_variables, shard, dist_h=True), self._ck(matrices)
        part = PartialC()
        lb = self._ctx.lib
        if z_dev_ptr:
            n_assign = matrices.num_instance_variables + matrices.num_witness_variables
            lb.check(lb.c.g16_prove_partial_h(self._ctx.handle, dpk.handle, dck.handle, C.c_void_p(z_dev_ptr), n_assign, 1, C.c_void_p(h_dev_ptr),
                                              h_len, int(skip_b_g1), C.byref(part)))
            return bytes(part)
        z = _c(full_assignment)
        lb.check(lb.c.g16_prove_partial_h(self._ctx.handle, dpk.handle, dck.handle, z.ctypes.data, z.shape[0], 0, C.c_void_p(h_dev_ptr), h_len,
                                          int(skip_b_g1), C.byref(part)))
        return bytes(part)

    def prove_finalize(self, pk: ProvingKey, num_inputs: int, parts: Sequence[bytes], r: np.ndarray, s: np.ndarray,
                       shard: Tuple[int, int] = (0, 1), dist_h: bool = False) -> Proof:
        _host_key(pk, "prove_finalize")
        L = FQ_LIMBS[self.curve]
        dpk = self._pk(pk, num_inputs, shard, dist_h)   # any shard carries the eight fixed points the glue reads
        arr = (PartialC * len(parts))(*[PartialC.from_buffer_copy(p) for p in parts])
        out = ProofC()
        lb = self._ctx.lib
        lb.check(lb.c.g16_prove_finalize(self._ctx.handle, dpk.handle, arr, len(parts), ptr64(_c(r)), ptr64(_c(s)), C.byref(out)))
        return Proof(np.array(out.a[: 2 * L], dtype=np.uint64), np.array(out.b[: 4 * L], dtype=np.uint64),
                     np.array(out.c[: 2 * L], dtype=np.uint64))


def rerandomize_proof(curve: str, vk: "ProvingKey", proof: "Proof", rng=None) -> "Proof":
    """Groth16::rerandomize_proof (prover.rs:223-250): A' = (1/r1) A, B' = r1 B + r1 r2 delta_g2, C' = C + r2 A for fresh
    non-zero r1, r2 (figure 1 of BKSV20).  Three scalar multiplications: host work, through the library's host field / group
    code -- no GPU context needed."""
    lb, cid, L = lib(), CURVE_ID[curve], FQ_LIMBS[curve]
    r1, r2 = _rand_fr(curve, rng, nonzero=True), _rand_fr(curve, rng, nonzero=True)

    def fr(op, a, b=None):   # g16_host_field_op on Fr: 2 mul, 3 inverse, 4 to_canonical
        out = np.zeros(4, dtype=np.uint64)
        lb.check(lb.c.g16_host_field_op(cid, 0, op, ptr64(_c(a)), ptr64(_c(b)) if b is not None else None, ptr64(out)))
        return out

    def grp(g2, op, p, q):   # g16_host_group_op: 0 p + q, 1 k * p (k canonical)
        out = np.zeros((4 if g2 else 2) * L, dtype=np.uint64)
        lb.check(lb.c.g16_host_group_op(cid, int(g2), op, ptr64(_c(p).reshape(-1)), ptr64(_c(q).reshape(-1)), ptr64(out)))
        return out

    canon = lambda x: fr(4, x)  # noqa: E731
    new_a = grp(False, 1, proof.a, canon(fr(3, r1)))
    new_b = grp(True, 0, grp(True, 1, proof.b, canon(r1)), grp(True, 1, vk.delta_g2, canon(fr(2, r1, r2))))
    new_c = grp(False, 0, proof.c, grp(False, 1, proof.a, canon(r2)))
    return Proof(new_a, new_b, new_c)


def fixed_points_view(pk: "ProvingKey"):
    """g16_pk_view with only the eight fixed points filled (what g16_finalize_host reads); returns (view, keepalive)"""
    keep = [_c(x).reshape(-1) for x in (pk.alpha_g1, pk.beta_g1, pk.delta_g1, pk.beta_g2, pk.delta_g2, pk.a_query[0], pk.b_g1_query[0],
                                        pk.b_g2_query[0])]
    empty = QueryC(None, 0, 0)
    return PkViewC(*[ptr64(k) for k in keep], empty, empty, empty, empty, empty, 0), keep


def finalize_host(curve: str, pk: "ProvingKey", parts: Sequence[bytes], r: np.ndarray, s: np.ndarray) -> "Proof":
    """g16_finalize_host: N-way EC fold of shard records + the prover.rs:76-131 glue, no GPU needed"""
    _host_key(pk, "finalize_host")
    L = FQ_LIMBS[curve]
    view, keep = fixed_points_view(pk)
    arr = (PartialC * len(parts))(*[PartialC.from_buffer_copy(p) for p in parts])
    out = ProofC()
    lb = lib()
    lb.check(lb.c.g16_finalize_host(CURVE_ID[curve], C.byref(view), arr, len(parts), ptr64(_c(r)), ptr64(_c(s)), C.byref(out)))
    return Proof(np.array(out.a[: 2 * L], dtype=np.uint64), np.array(out.b[: 4 * L], dtype=np.uint64), np.array(out.c[: 2 * L], dtype=np.uint64))


class DistributedWitnessMap:
    """g16_dwm_*: one rank's side of the distributed witness map (h = witness_map_from_matrices, r1cs_to_qap.rs:172-235, with
    every n-point transform cut into a local n/world-point transform, a twiddle, ONE all-to-all and a local world-point
    transform).  The object owns the rank's device buffers (torch tensors: work[3], recv[3], h_local, M = n / world Fr each);
    the caller owns the exchange -- `run` does it with torch.distributed.all_to_all_single (RCCL over xGMI for backend
    "nccl"), the single-process tests move the chunks themselves between the ranks' objects."""

    def __init__(self, lib_, ctx_handle, circuit_handle, rank: int, world: int, device):
        import torch

        self.lib, self.ctx, self.rank, self.world = lib_, ctx_handle, rank, world
        self.handle = C.c_void_p()
        lib_.check(lib_.c.g16_dwm_create(ctx_handle, circuit_handle, rank, world, C.byref(self.handle)))
        self.M = int(lib_.c.g16_dwm_local_size(self.handle))
        self.blk = self.M // world
        mk = lambda: torch.empty((self.M, 4), dtype=torch.int64, device=device)  # noqa: E731
        self.work, self.recv, self.h_local = [mk() for _ in range(3)], [mk() for _ in range(3)], mk()
        self.h_full = None   # all_gather_h: the n-element buffer of a bucket-space shard
        self._wp = (C.c_void_p * 3)(*[t.data_ptr() for t in self.work])
        self._rp = (C.c_void_p * 3)(*[t.data_ptr() for t in self.recv])

    def stage(self, s: int, z_ptr: int = 0, n_assign: int = 0, on_device: bool = False):
        """stage 0: full_assignment -> work[0..2];  1: recv[0..2] -> work[0..2];  2: recv[0..2] -> work[0];  3: recv[0] -> h_local.
        Returns with the device work finished."""
        self.lib.check(self.lib.c.g16_dwm_stage(self.ctx, self.handle, s, C.c_void_p(z_ptr) if z_ptr else None, n_assign, int(on_device),
                                                self._wp, self._rp, C.c_void_p(self.h_local.data_ptr())))

    @staticmethod
    def arrays_after(s: int) -> int:
        """arrays exchanged after stage s (a, b, c after stages 0 and 1; the quotient after stage 2)"""
        return 3 if s < 2 else 1

    def stage_async(self, s: int, z_dev_ptr: int = 0, n_assign: int = 0):
        """g16_dwm_stage_async: the stage is enqueued on the context's witness-map stream and the call returns"""
        self.lib.check(self.lib.c.g16_dwm_stage_async(self.ctx, self.handle, s, C.c_void_p(z_dev_ptr) if z_dev_ptr else None, n_assign,
                                                      self._wp, self._rp, C.c_void_p(self.h_local.data_ptr())))

    def run(self, z_ptr: int, n_assign: int, on_device: bool, dist):
        """all four stages with the exchanges over `dist` (torch.distributed); returns h_local.

        Device-resident assignment + RCCL (or a single rank): NOTHING here waits on the host -- stages (g16_dwm_stage_async) and
        exchanges (all_to_all_single: chunk p of work -> rank p, the chunk from rank q -> position q of recv) are enqueued on the
        library's witness-map stream, which torch adopts as an external stream; the three arrays of an exchange step go
        back to back.  A following prove_partial_h orders only its h sort / h MSM after this stream.  Otherwise (host assignment, or
        gloo in the one-GPU / CPU tests, which has no all-to-all): stage by stage with host synchronisation."""
        import torch

        import os

        # G16_DWM_FORCE_COLLECTIVE (test-only): issue the collective with one rank too, so that a one-GPU box exercises
        # all_to_all_single over RCCL on the adopted stream exactly as the N > 1 runs do
        multi = dist is not None and (self.world > 1 or bool(os.environ.get("G16_DWM_FORCE_COLLECTIVE")))
        if on_device and (not multi or dist.get_backend() == "nccl"):
            ext = torch.cuda.ExternalStream(int(self.lib.c.g16_ctx_wm_stream(self.ctx)), device=self.h_local.device)
            with torch.cuda.stream(ext):
                for s in range(4):
                    self.stage_async(s, z_ptr if s == 0 else 0, n_assign if s == 0 else 0)
                    if s < 3:
                        for m in range(self.arrays_after(s)):
                            if multi:
                                dist.all_to_all_single(self.recv[m], self.work[m])
                            else:
                                self.recv[m].copy_(self.work[m])
            return self.h_local
        for s in range(4):
            self.stage(s, z_ptr if s == 0 else 0, n_assign if s == 0 else 0, on_device)
            if s < 3:
                for m in range(self.arrays_after(s)):
                    src, dst = self.work[m], self.recv[m]
                    if multi:
                        if dist.get_backend() == "nccl":
                            dist.all_to_all_single(dst, src)      # chunk p of src -> rank p; chunk from rank q -> position q
                        else:   # gloo (one-GPU / CPU tests) has no all-to-all: gather everything on the host, keep my chunks
                            mine = src.cpu()
                            every = [torch.empty_like(mine) for _ in range(self.world)]
                            dist.all_gather(every, mine)
                            blk = self.blk
                            dst.copy_(torch.cat([e[self.rank * blk:(self.rank + 1) * blk] for e in every]))
                    else:
                        dst.copy_(src)
                torch.cuda.synchronize()   # the next stage runs on the library's own stream
        return self.h_local

    def all_gather_h(self, dist=None, simulate: bool = False):
        """h WHOLE on this rank, for a bucket-space shard (every rank runs the h MSM over all coefficients and 1 / world of the
        buckets): ONE all-gather of the ranks' blocks (n / world Fr each -- 16 MiB per rank at 2^22 / 8) into an n-element buffer, in
        rank order -- the order `bucket_h_indices` lists and the key's h_query is loaded in, so nothing is un-permuted.  With RCCL
        (or one rank, or `simulate`: this rank's block copied `world` times -- the same bytes written, for the one-GPU share
        measurement) the gather is enqueued on the witness-map stream behind the map's last stage, with no host synchronisation;
        a following prove_partial_h orders itself after that stream.  gloo (tests): through the host."""
        import torch

        if getattr(self, "h_full", None) is None:
            self.h_full = torch.empty((self.M * self.world, 4), dtype=torch.int64, device=self.h_local.device)
        multi = dist is not None and self.world > 1 and not simulate
        if multi and dist.get_backend() != "nccl":
            torch.cuda.synchronize()
            mine = self.h_local.cpu()
            every = [torch.empty_like(mine) for _ in range(self.world)]
            dist.all_gather(every, mine)
            self.h_full.copy_(torch.cat(every))
            torch.cuda.synchronize()
            return self.h_full
        ext = torch.cuda.ExternalStream(int(self.lib.c.g16_ctx_wm_stream(self.ctx)), device=self.h_local.device)
        with torch.cuda.stream(ext):
            if multi:
                dist.all_gather_into_tensor(self.h_full, self.h_local)
            else:
                for q in range(self.world):
                    self.h_full[q * self.M:(q + 1) * self.M].copy_(self.h_local, non_blocking=True)
        return self.h_full

    def close(self):
        if self.handle:
            self.lib.c.g16_dwm_free(self.handle)
            self.handle = C.c_void_p()
        self.h_full = None


class PipelinedProver:
    """Throughput mode on one GPU: two contexts over ONE device-resident key / circuit, two worker threads.  `submit` returns a
    `concurrent.futures.Future` of the proof; with two proofs in flight the witness map / sort of one and the reductions / host glue of
    the other run under each other's bucket passes (bench.py reports the effect as `pipelined`: +3.9 % proofs per second at 2^22).
    Latency per proof roughly doubles -- use a plain `Groth16` when that matters.  `qap` as for `Groth16`."""

    def __init__(self, curve: str = "bls12_381", device: int = 0, qap=LibsnarkReduction):
        import queue
        import threading

        self._owner = Groth16(curve, device, qap=qap)
        self._second = Groth16(curve, device, qap=qap)
        self._second.share_device_data_of(self._owner)
        self._lock = threading.Lock()           # key / circuit loads go through the owner's caches: one at a time
        self._idle = threading.Condition()      # _busy: proofs in flight (a Circom circuit's C is attached only between proofs)
        self._busy = 0
        self._jobs: "queue.Queue" = queue.Queue()
        self._threads = [threading.Thread(target=self._work, args=(p,), daemon=True) for p in (self._owner, self._second)]
        for t in self._threads:
            t.start()

    def _work(self, prover: Groth16):
        while True:
            job = self._jobs.get()
            if job is None:
                return
            fut, args = job
            if not fut.set_running_or_notify_cancel():
                continue
            try:
                pk, r, s, matrices, num_inputs, num_constraints, z, check = args
                with self._lock:     # make sure the handles exist (first use loads them) before the unlocked, concurrent proof
                    prover._pk(pk, num_inputs)
                    if check and not prover._ck(matrices)._has_c:
                        # attaching C changes the circuit both contexts read: not while the other worker is proving over it
                        with self._idle:
                            self._idle.wait_for(lambda: self._busy == 0)
                            prover._ck(matrices, for_check=True)
                    with self._idle:
                        self._busy += 1
                try:
                    fut.set_result(prover.create_proof_with_reduction_and_matrices(pk, r, s, matrices, num_inputs, num_constraints, z, check=check))
                finally:
                    with self._idle:
                        self._busy -= 1
                        self._idle.notify_all()
            except BaseException as e:  # noqa: BLE001 -- delivered through the future
                fut.set_exception(e)

    def submit(self, pk: ProvingKey, r: np.ndarray, s: np.ndarray, matrices: ConstraintMatrices, num_inputs: int, num_constraints: int,
               full_assignment: np.ndarray, check: bool = False):
        """Groth16::create_proof_with_reduction_and_matrices (prover.rs:26-51), asynchronously; check as there (the future then
        carries `Unsatisfiable` for a bad assignment)"""
        from concurrent.futures import Future

        fut: Future = Future()
        self._jobs.put((fut, (pk, r, s, matrices, num_inputs, num_constraints, full_assignment, check)))
        return fut

    def close(self):
        for _ in self._threads:
            self._jobs.put(None)
        for t in self._threads:
            t.join()
        self._second.close()
        self._owner.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class ShardedProver:
    """One process per GPU: every rank holds a contiguous shard of each MSM base array, computes its
    partial sums, and the fixed-size records are exchanged with ONE all-gather (RCCL over xGMI when
    the process group backend is "nccl"; gloo in the CPU tests).  Group addition is not an
    element-wise sum, so the collective is an all-gather of ~1.2 KB per rank followed by a local
    N-way EC addition inside g16_prove_finalize -- not an all-reduce.  The witness map is
    replicated (it is ~5 % of a single-GPU proof)."""

    PARTIAL_BYTES = C.sizeof(PartialC)

    def __init__(self, prover: Groth16, pk: ProvingKey, matrices: ConstraintMatrices, rank: int, world_size: int, mode: str = "base"):
        """mode "base": contiguous ranges of the bases per rank (1 / world of the key's memory per GPU); "bucket": the whole key
        on every GPU, the BUCKETS divided (b mod world == rank) -- the bucket reductions then shrink with the rank count too
        (g16_pk_load_bucket_shard)"""
        if mode not in ("base", "bucket"):
            raise ValueError("mode is 'base' or 'bucket'")
        _host_key(pk, "ShardedProver")
        self.prover, self.pk, self.matrices = prover, pk, matrices
        self.rank, self.world, self.mode = rank, world_size, mode
        self.shard = (rank, world_size, "bucket") if mode == "bucket" and world_size > 1 else (rank, world_size)

    def local_partial(self, full_assignment: np.ndarray, r: np.ndarray) -> bytes:
        return self.prover.prove_partial(self.pk, self.matrices, full_assignment, self.shard, skip_b_g1=not np.asarray(r).any())

    @staticmethod
    def exchange(local: bytes, dist, device=None) -> List[bytes]:
        """all-gather of the partial records through torch.distributed"""
        import torch

        t = torch.frombuffer(bytearray(local), dtype=torch.uint8)
        if device is not None:
            t = t.to(device)
        outs = [torch.empty_like(t) for _ in range(dist.get_world_size())]
        dist.all_gather(outs, t)
        return [bytes(o.cpu().numpy().tobytes()) for o in outs]

    def prove(self, full_assignment: np.ndarray, r: np.ndarray, s: np.ndarray, dist=None, device=None) -> Proof:
        local = self.local_partial(full_assignment, r)
        parts = [local] if (dist is None or self.world == 1) else self.exchange(local, dist, device)
        return self.prover.prove_finalize(self.pk, self.matrices.num_instance_variables, parts, r, s, self.shard)
