"""Groth16 verification (src/verifier.rs:13-76, src/lib.rs:84-96) through the library's pairing: the batch form runs one proof per
GPU lane (g16_verify_batch); ``verify_proof_host`` runs the same C++ templates on the CPU (g16_host_verify).  The aggregate form
(g16_verify_aggregate / g16_host_verify_aggregate) checks a whole batch under one key in one randomised equation; the mixed form
(g16_verify_aggregate_mixed / g16_host_verify_aggregate_mixed) does so for a batch whose proofs name their keys."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
import numpy as np

from .binding import CURVE_ID, FQ_LIMBS, VkViewC, lib, ptr32, ptr64


def _c(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint64))


@dataclass
class VerifyingKey:
    """src/data_structures.rs:31-44; affine Montgomery limbs (gamma_abc_g1: (n, 2 * FQ) array)."""

    curve: str
    alpha_g1: np.ndarray
    beta_g2: np.ndarray
    gamma_g2: np.ndarray
    delta_g2: np.ndarray
    gamma_abc_g1: np.ndarray

    @staticmethod
    def from_proving_key(pk) -> "VerifyingKey":
        if pk.gamma_g2 is None or pk.gamma_abc_g1 is None:
            raise ValueError("this ProvingKey carries no gamma_g2 / gamma_abc_g1 (a key made by setup() or generate_parameters has them)")
        return VerifyingKey(pk.curve, _c(pk.alpha_g1), _c(pk.beta_g2), _c(pk.gamma_g2), _c(pk.delta_g2), _c(pk.gamma_abc_g1))

    def view(self):
        """(g16_vk_view, the arrays it points into)"""
        L = FQ_LIMBS[self.curve]
        keep = [_c(self.alpha_g1).reshape(-1), _c(self.beta_g2).reshape(-1), _c(self.gamma_g2).reshape(-1), _c(self.delta_g2).reshape(-1),
                _c(self.gamma_abc_g1).reshape(-1, 2 * L)]
        v = VkViewC(*[ptr64(a) for a in keep], keep[4].shape[0])
        return v, keep

    @property
    def num_public(self) -> int:
        return _c(self.gamma_abc_g1).reshape(-1, 2 * FQ_LIMBS[self.curve]).shape[0] - 1


def as_vk(vk) -> VerifyingKey:
    return vk if isinstance(vk, VerifyingKey) else VerifyingKey.from_proving_key(vk)


class PreparedVerifyingKey:
    """src/data_structures.rs:56-66: owns the device-resident g16_pvk (e(alpha, beta), the prepared lines of -gamma and -delta,
    the window tables of gamma_abc_g1) of one context."""

    def __init__(self, ctx, vk):
        self.vk = as_vk(vk)
        self.curve = self.vk.curve
        self._ctx = ctx
        self.handle = C.c_void_p()
        view, keep = self.vk.view()
        lb = lib()
        lb.check(lb.c.g16_pvk_load(ctx.handle, C.byref(view), C.byref(self.handle)))
        del keep

    @property
    def alpha_g1_beta_g2(self) -> np.ndarray:
        """GT value as arkworks' 12 Fq (Montgomery limbs), c0.c0.c0 ... c1.c2.c1"""
        out = np.zeros(12 * FQ_LIMBS[self.curve], dtype=np.uint64)
        lb = lib()
        lb.check(lb.c.g16_pvk_alpha_beta(self.handle, ptr64(out)))
        return out

    def close(self):
        if self.handle:
            lib().c.g16_pvk_free(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _flat_proofs(proofs, curve) -> np.ndarray:
    L = FQ_LIMBS[curve]
    if isinstance(proofs, np.ndarray):
        return _c(proofs).reshape(-1, 8 * L)
    if not len(proofs):
        return np.zeros((0, 8 * L), np.uint64)
    return _c(np.stack([p if isinstance(p, np.ndarray) else p.flat() for p in proofs])).reshape(-1, 8 * L)


def verify_batch(ctx, pvk: PreparedVerifyingKey, proofs, public_inputs_list) -> np.ndarray:
    """verdict bytes: 1 accept, 0 reject, 2 a proof point is not on its curve"""
    flat = _flat_proofs(proofs, pvk.curve)
    n = flat.shape[0]
    x, num_public = _flat_inputs(public_inputs_list, n, pvk.vk.num_public)
    verdicts = np.zeros(n, dtype=np.uint8)
    lb = lib()
    lb.check(lb.c.g16_verify_batch(ctx.handle, pvk.handle, ptr64(flat.reshape(-1)), n, ptr64(x) if x.size else None, num_public,
                                   verdicts.ctypes.data_as(C.c_void_p)))
    return verdicts


def _flat_inputs(public_inputs_list, n, default_num_public):
    """(flat words, inputs per proof) of one vector of Fr rows per proof; an (n, num_public, 4) uint64 array is taken as it is"""
    if len(public_inputs_list) != n:
        raise ValueError("one public-input vector per proof")
    if isinstance(public_inputs_list, np.ndarray) and public_inputs_list.dtype == np.uint64 and public_inputs_list.ndim == 3 and n:
        if public_inputs_list.shape[2] != 4:
            raise ValueError("an Fr element is 4 words")
        return np.ascontiguousarray(public_inputs_list).reshape(-1), public_inputs_list.shape[1]
    rows = [_c(x).reshape(-1, 4) if len(x) else np.zeros((0, 4), dtype=np.uint64) for x in public_inputs_list]
    num_public = rows[0].shape[0] if n else default_num_public
    if any(r.shape[0] != num_public for r in rows):
        raise ValueError("every proof of a batch needs the same number of public inputs")
    x = np.ascontiguousarray(np.concatenate(rows).reshape(-1)) if n and num_public else np.zeros(0, dtype=np.uint64)
    return x, num_public


def _flat_coeffs(coeffs, n):
    """None, or n 128-bit coefficients (Python ints, or an (n, 2) array of little-endian 64-bit words) as n x 2 words"""
    if coeffs is None:
        return None
    if isinstance(coeffs, np.ndarray) and coeffs.dtype == np.uint64:
        out = _c(coeffs).reshape(-1, 2)
    else:
        ints = [int(r) for r in coeffs]
        if any(r < 0 or r >> 128 for r in ints):
            raise ValueError("a coefficient is a 128-bit unsigned integer")
        out = np.array([[r & (2**64 - 1), r >> 64] for r in ints], dtype=np.uint64).reshape(-1, 2)
    if out.shape[0] != n:
        raise ValueError("one coefficient per proof")
    return np.ascontiguousarray(out)


def verify_aggregate(ctx, pvk: PreparedVerifyingKey, proofs, public_inputs_list, coeffs=None, check_subgroups: bool = False) -> int:
    """g16_verify_aggregate's verdict: 1 every proof holds, 0 the aggregate equation fails, 2 a point is off its curve.
    check_subgroups=True goes through g16_verify_aggregate_checked, which adds 3: a point is on its curve but outside its
    prime-order subgroup"""
    flat = _flat_proofs(proofs, pvk.curve)
    n = flat.shape[0]
    x, num_public = _flat_inputs(public_inputs_list, n, pvk.vk.num_public)
    r = _flat_coeffs(coeffs, n)
    v = np.zeros(1, dtype=np.uint8)
    lb = lib()
    fn = lb.c.g16_verify_aggregate_checked if check_subgroups else lb.c.g16_verify_aggregate
    lb.check(fn(ctx.handle, pvk.handle, ptr64(flat.reshape(-1)) if n else None, n, ptr64(x) if x.size else None, num_public,
                ptr64(r.reshape(-1)) if r is not None and n else None, v.ctypes.data_as(C.c_void_p)))
    return int(v[0])


def _flat_points(points, curve, g2) -> np.ndarray:
    return _c(points).reshape(-1, (4 if g2 else 2) * FQ_LIMBS[curve])


def check_subgroups(ctx, points, g2: bool = False) -> np.ndarray:
    """g16_check_subgroups: a byte per affine point (G1, or G2 with g2=True) -- 1 in the prime-order subgroup, 0 on the curve
    but outside it, 2 off the curve"""
    flat = _flat_points(points, ctx.curve, g2)
    flags = np.zeros(flat.shape[0], dtype=np.uint8)
    lb = lib()
    lb.check(lb.c.g16_check_subgroups(ctx.handle, int(bool(g2)), ptr64(flat.reshape(-1)) if flat.size else None, flat.shape[0],
                                      flags.ctypes.data_as(C.c_void_p)))
    return flags


def check_proof_subgroups(ctx, proofs) -> np.ndarray:
    """g16_check_proof_subgroups: a byte per proof -- 2 if A, B or C is off its curve, otherwise 0 if one of them is outside its
    subgroup, otherwise 1"""
    flat = _flat_proofs(proofs, ctx.curve)
    flags = np.zeros(flat.shape[0], dtype=np.uint8)
    lb = lib()
    lb.check(lb.c.g16_check_proof_subgroups(ctx.handle, ptr64(flat.reshape(-1)) if flat.size else None, flat.shape[0],
                                            flags.ctypes.data_as(C.c_void_p)))
    return flags


def _encoded(data, size: int) -> np.ndarray:
    """bytes or a uint8 array as a contiguous uint8 vector holding whole encodings of `size` bytes"""
    if isinstance(data, np.ndarray):
        if data.dtype != np.uint8:
            raise ValueError("encoded points are bytes or a uint8 array")
        a = np.ascontiguousarray(data).reshape(-1)
    else:
        a = np.frombuffer(bytes(data), dtype=np.uint8)
    if a.size % size:
        raise ValueError(f"{a.size} bytes are no whole number of {size}-byte encodings")
    return a


def _fq_bytes(curve: str) -> int:
    return 48 if curve == "bls12_381" else 32


def _u8ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p) if a.size else None


def decompress_points(ctx, data, g2: bool = False):
    """g16_decompress_points: packed compressed points (G1, or G2 with g2=True) decoded on the GPU by the rules of
    deserialize_points(compressed=True, validate=0).  (points, status): affine Montgomery limbs per point and a byte per point --
    1 decoded, 0 an invalid encoding (its point is the identity)"""
    L = FQ_LIMBS[ctx.curve]
    enc = _encoded(data, _fq_bytes(ctx.curve) * (2 if g2 else 1))
    n = enc.size // (_fq_bytes(ctx.curve) * (2 if g2 else 1))
    out = np.zeros((n, (4 if g2 else 2) * L), dtype=np.uint64)
    status = np.zeros(n, dtype=np.uint8)
    lb = lib()
    lb.check(lb.c.g16_decompress_points(ctx.handle, int(bool(g2)), _u8ptr(enc), n, ptr64(out.reshape(-1)) if n else None, _u8ptr(status)))
    return out, status


def decompress_proofs(ctx, data):
    """g16_decompress_proofs: n compressed proofs A | B | C (proof_to_bytes(compressed=True)) decoded on the GPU.
    (flat_proofs, status): n x (A | B | C) affine as verify_batch takes them, and a byte per proof -- 1 iff A, B and C all decode"""
    L = FQ_LIMBS[ctx.curve]
    enc = _encoded(data, 4 * _fq_bytes(ctx.curve))
    n = enc.size // (4 * _fq_bytes(ctx.curve))
    out = np.zeros((n, 8 * L), dtype=np.uint64)
    status = np.zeros(n, dtype=np.uint8)
    lb = lib()
    lb.check(lb.c.g16_decompress_proofs(ctx.handle, _u8ptr(enc), n, ptr64(out.reshape(-1)) if n else None, _u8ptr(status)))
    return out, status


def decompress_points_host(curve: str, data, g2: bool = False):
    """decompress_points on the CPU through g16_host_decompress_points (the same C++ templates, no GPU): (points, status)"""
    L = FQ_LIMBS[curve]
    size = _fq_bytes(curve) * (2 if g2 else 1)
    enc = _encoded(data, size)
    n = enc.size // size
    out = np.zeros((n, (4 if g2 else 2) * L), dtype=np.uint64)
    status = np.zeros(n, dtype=np.uint8)
    lb = lib()
    lb.check(lb.c.g16_host_decompress_points(CURVE_ID[curve], int(bool(g2)), _u8ptr(enc), n, ptr64(out.reshape(-1)) if n else None,
                                             _u8ptr(status)))
    return out, status


def _decode_points(call, curve: str, data, g2: bool, compressed: bool, validate: int):
    L = FQ_LIMBS[curve]
    size = _fq_bytes(curve) * (2 if g2 else 1) * (1 if compressed else 2)
    enc = _encoded(data, size)
    n = enc.size // size
    out = np.zeros((n, (4 if g2 else 2) * L), dtype=np.uint64)
    status = np.zeros(n, dtype=np.uint8)
    lib().check(call(int(bool(g2)), int(bool(compressed)), int(validate), _u8ptr(enc), n, ptr64(out.reshape(-1)) if n else None, _u8ptr(status)))
    return out, status


def decode_points(ctx, data, g2: bool = False, compressed: bool = True, validate: int = 2):
    """g16_decode_points: packed encodings (either form) decoded and validated on the GPU, point by point what
    deserialize_points(compressed, validate) does to each.  (points, status): status 1 and the point where that call accepts it,
    else the identity and 0 the bytes do not decode / 2 off the curve / 3 outside the prime-order subgroup"""
    return _decode_points(lambda *a: lib().c.g16_decode_points(ctx.handle, *a), ctx.curve, data, g2, compressed, validate)


def decode_points_host(curve: str, data, g2: bool = False, compressed: bool = True, validate: int = 2):
    """decode_points on the CPU through g16_host_decode_points (the same C++ templates, no GPU): (points, status)"""
    return _decode_points(lambda *a: lib().c.g16_host_decode_points(CURVE_ID[curve], *a), curve, data, g2, compressed, validate)


def verify_aggregate_bytes(ctx, pvk: PreparedVerifyingKey, data, public_inputs_list, coeffs=None) -> int:
    """g16_verify_aggregate_bytes' verdict over compressed proofs, decoded and membership-tested on the GPU: 1 every proof holds,
    0 the aggregate equation fails, 3 a point is outside its prime-order subgroup, 4 some proof's bytes do not decode (4 wins over 3)"""
    enc = _encoded(data, 4 * _fq_bytes(pvk.curve))
    n = enc.size // (4 * _fq_bytes(pvk.curve))
    x, num_public = _flat_inputs(public_inputs_list, n, pvk.vk.num_public)
    r = _flat_coeffs(coeffs, n)
    v = np.zeros(1, dtype=np.uint8)
    lb = lib()
    lb.check(lb.c.g16_verify_aggregate_bytes(ctx.handle, pvk.handle, _u8ptr(enc), n, ptr64(x) if x.size else None, num_public,
                                             ptr64(r.reshape(-1)) if r is not None and n else None, v.ctypes.data_as(C.c_void_p)))
    return int(v[0])


def _host_aggregate_args(curve, vk, proofs, public_inputs_list, coeffs):
    vkk = as_vk(vk)
    flat = _flat_proofs(proofs, curve)
    n = flat.shape[0]
    x, num_public = _flat_inputs(public_inputs_list, n, vkk.num_public)
    r = _flat_coeffs(coeffs, n)
    view, keep = vkk.view()
    args = (CURVE_ID[curve], C.byref(view), ptr64(flat.reshape(-1)) if n else None, n, ptr64(x) if x.size else None, num_public,
            ptr64(r.reshape(-1)) if r is not None and n else None)
    return args, (view, keep, flat, x, r)


def host_aggregate_verdict(curve: str, vk, proofs, public_inputs_list, coeffs=None) -> int:
    """g16_host_verify_aggregate's verdict byte (1 / 0 / 2)"""
    args, keep = _host_aggregate_args(curve, vk, proofs, public_inputs_list, coeffs)
    v = np.zeros(1, dtype=np.uint8)
    lb = lib()
    lb.check(lb.c.g16_host_verify_aggregate(*args, v.ctypes.data_as(C.c_void_p)))
    del keep
    return int(v[0])


def verify_proofs_aggregate_host(curve: str, vk, proofs, public_inputs_list, coeffs=None) -> bool:
    """the randomised batch equation on the CPU: True iff every proof of the batch is accepted (see g16_verify_aggregate for the
    soundness contract); coeffs=None draws the coefficients from the operating system"""
    return host_aggregate_verdict(curve, vk, proofs, public_inputs_list, coeffs) == 1


def host_aggregate_gt(curve: str, vk, proofs, public_inputs_list, coeffs):
    """(lhs, rhs): the two GT values the aggregate equation compares, as arkworks' 12 Fq limbs"""
    args, keep = _host_aggregate_args(curve, vk, proofs, public_inputs_list, coeffs)
    L = FQ_LIMBS[curve]
    lhs, rhs = np.zeros(12 * L, dtype=np.uint64), np.zeros(12 * L, dtype=np.uint64)
    lb = lib()
    lb.check(lb.c.g16_host_verify_aggregate_gt(*args, ptr64(lhs), ptr64(rhs)))
    del keep
    return lhs, rhs


def _mixed_args(curve, key_of, proofs, public_inputs_list, coeffs):
    """(key_of, flat proofs, n, ragged inputs as flat words, their count in Fr, coefficients) of a mixed batch.  A proof's input
    vector is passed on as it is: whether its length suits its key is the library's check (G16_ERR_MALFORMED_VK)"""
    flat = _flat_proofs(proofs, curve)
    n = flat.shape[0]
    ko = np.ascontiguousarray(np.asarray(key_of, dtype=np.int64).reshape(-1))
    if ko.shape[0] != n:
        raise ValueError("one key index per proof")
    if n and (ko.min() < 0 or ko.max() >> 32):
        raise ValueError("a key index is a 32-bit unsigned integer")
    ko = ko.astype(np.uint32)
    if len(public_inputs_list) != n:
        raise ValueError("one public-input vector per proof")
    if isinstance(public_inputs_list, np.ndarray) and public_inputs_list.dtype == np.uint64 and public_inputs_list.ndim == 3:
        if public_inputs_list.shape[2] != 4:   # (n, l, 4): every key of the batch takes l inputs
            raise ValueError("an Fr element is 4 words")
        x = np.ascontiguousarray(public_inputs_list).reshape(-1)
    else:
        rows = [_c(x).reshape(-1, 4) if len(x) else np.zeros((0, 4), dtype=np.uint64) for x in public_inputs_list]
        x = np.ascontiguousarray(np.concatenate(rows).reshape(-1)) if rows else np.zeros(0, dtype=np.uint64)
    return ko, flat, n, x, x.size // 4, _flat_coeffs(coeffs, n)


def verify_aggregate_mixed(ctx, pvks, key_of, proofs, public_inputs_list, coeffs=None, check_subgroups: bool = False) -> int:
    """g16_verify_aggregate_mixed's verdict for proofs made under several keys (key_of[i] indexes pvks): 1 every proof holds under
    its key, 0 the aggregate equation fails, 2 a point is off its curve, 3 (check_subgroups=True) a point is outside its subgroup"""
    pvks = list(pvks)
    curve = ctx.curve
    ko, flat, n, x, n_public_total, r = _mixed_args(curve, key_of, proofs, public_inputs_list, coeffs)
    handles = (C.c_void_p * max(len(pvks), 1))(*[p.handle if p is not None else None for p in pvks])
    v = np.zeros(1, dtype=np.uint8)
    lb = lib()
    lb.check(lb.c.g16_verify_aggregate_mixed(ctx.handle, handles, len(pvks), ptr32(ko) if n else None, ptr64(flat.reshape(-1)) if n else None, n,
                                             ptr64(x) if x.size else None, n_public_total, ptr64(r.reshape(-1)) if r is not None and n else None,
                                             int(bool(check_subgroups)), v.ctypes.data_as(C.c_void_p)))
    return int(v[0])


def _host_mixed_args(curve, vks, key_of, proofs, public_inputs_list, coeffs):
    vkks = [as_vk(vk) for vk in vks]
    ko, flat, n, x, n_public_total, r = _mixed_args(curve, key_of, proofs, public_inputs_list, coeffs)
    views = [vk.view() for vk in vkks]
    arr = (VkViewC * max(len(views), 1))(*[v for v, _ in views])
    args = (CURVE_ID[curve], arr, len(views), ptr32(ko) if n else None, ptr64(flat.reshape(-1)) if n else None, n,
            ptr64(x) if x.size else None, n_public_total, ptr64(r.reshape(-1)) if r is not None and n else None)
    return args, (views, arr, ko, flat, x, r)


def host_aggregate_mixed_verdict(curve: str, vks, key_of, proofs, public_inputs_list, coeffs=None) -> int:
    """g16_host_verify_aggregate_mixed's verdict byte (1 / 0 / 2)"""
    args, keep = _host_mixed_args(curve, vks, key_of, proofs, public_inputs_list, coeffs)
    v = np.zeros(1, dtype=np.uint8)
    lb = lib()
    lb.check(lb.c.g16_host_verify_aggregate_mixed(*args, v.ctypes.data_as(C.c_void_p)))
    del keep
    return int(v[0])


def verify_proofs_aggregate_mixed_host(curve: str, vks, key_of, proofs, public_inputs_list, coeffs=None) -> bool:
    """the mixed-key aggregate equation on the CPU: True iff every proof of the batch is accepted under the key it names"""
    return host_aggregate_mixed_verdict(curve, vks, key_of, proofs, public_inputs_list, coeffs) == 1


def host_aggregate_mixed_gt(curve: str, vks, key_of, proofs, public_inputs_list, coeffs):
    """(lhs, rhs): the two GT values the mixed-key equation compares, as arkworks' 12 Fq limbs"""
    args, keep = _host_mixed_args(curve, vks, key_of, proofs, public_inputs_list, coeffs)
    L = FQ_LIMBS[curve]
    lhs, rhs = np.zeros(12 * L, dtype=np.uint64), np.zeros(12 * L, dtype=np.uint64)
    lb = lib()
    lb.check(lb.c.g16_host_verify_aggregate_mixed_gt(*args, ptr64(lhs), ptr64(rhs)))
    del keep
    return lhs, rhs


def verify_batch_prepared(ctx, pvk: PreparedVerifyingKey, proofs, prepared_inputs) -> np.ndarray:
    flat = _flat_proofs(proofs, pvk.curve)
    n = flat.shape[0]
    ic = _c(prepared_inputs).reshape(n, 2 * FQ_LIMBS[pvk.curve])
    verdicts = np.zeros(n, dtype=np.uint8)
    lb = lib()
    lb.check(lb.c.g16_verify_batch_prepared(ctx.handle, pvk.handle, ptr64(flat.reshape(-1)), ptr64(ic.reshape(-1)), n, verdicts.ctypes.data_as(C.c_void_p)))
    return verdicts


def verify_proof_host(curve: str, vk, proof, public_inputs) -> bool:
    """verify_proof (verifier.rs:68-76) on the CPU through g16_host_verify; raises MalformedVerifyingKey for a wrong input count.
    A proof with a point off its curve is rejected (False)."""
    return host_verdict(curve, vk, proof, public_inputs) == 1


def check_subgroups_host(curve: str, points, g2: bool = False) -> np.ndarray:
    """check_subgroups on the CPU through g16_host_check_subgroups (the same C++ templates, no GPU): 1 / 0 / 2 per point"""
    flat = _flat_points(points, curve, g2)
    flags = np.zeros(flat.shape[0], dtype=np.uint8)
    lb = lib()
    lb.check(lb.c.g16_host_check_subgroups(CURVE_ID[curve], int(bool(g2)), ptr64(flat.reshape(-1)) if flat.size else None, flat.shape[0],
                                           flags.ctypes.data_as(C.c_void_p)))
    return flags


def host_verdict(curve: str, vk, proof, public_inputs) -> int:
    """g16_host_verify's verdict byte (1 / 0 / 2)"""
    vkk = as_vk(vk)
    view, keep = vkk.view()
    x = _c(public_inputs).reshape(-1) if len(public_inputs) else np.zeros(0, dtype=np.uint64)
    flat = _c(proof if isinstance(proof, np.ndarray) else proof.flat()).reshape(-1)
    v = np.zeros(1, dtype=np.uint8)
    lb = lib()
    lb.check(lb.c.g16_host_verify(CURVE_ID[curve], C.byref(view), ptr64(flat), ptr64(x) if x.size else None, x.size // 4,
                                  v.ctypes.data_as(C.c_void_p)))
    del keep
    return int(v[0])


def host_pairing(curve: str, g1s, g2s) -> np.ndarray:
    """prod e(g1s[i], g2s[i]) on the CPU, as arkworks' 12 Fq limbs"""
    L = FQ_LIMBS[curve]
    a = _c(g1s).reshape(-1, 2 * L)
    b = _c(g2s).reshape(-1, 4 * L)
    out = np.zeros(12 * L, dtype=np.uint64)
    lb = lib()
    lb.check(lb.c.g16_host_pairing(CURVE_ID[curve], ptr64(a.reshape(-1)) if a.size else None, ptr64(b.reshape(-1)) if b.size else None,
                                   a.shape[0], ptr64(out)))
    return out


def device_pairing(ctx, g1s, g2s) -> np.ndarray:
    L = FQ_LIMBS[ctx.curve]
    a = _c(g1s).reshape(-1, 2 * L)
    b = _c(g2s).reshape(-1, 4 * L)
    out = np.zeros(12 * L, dtype=np.uint64)
    lb = lib()
    lb.check(lb.c.g16_pairing(ctx.handle, ptr64(a.reshape(-1)) if a.size else None, ptr64(b.reshape(-1)) if b.size else None, a.shape[0],
                              ptr64(out)))
    return out
