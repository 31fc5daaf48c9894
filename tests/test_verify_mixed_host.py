"""CPU tier: the aggregate equation for batches that mix verifying keys, on the host (g16_host_verify_aggregate_mixed runs the
templates g16_verify_aggregate_mixed uses) against the single-key call, the big-int model of the equation, per-proof verdicts and
the contract's error codes."""
import ctypes as C

import numpy as np
import pytest

import pairing_model as pmod
import pymodel as pm
from aggregate_cases import cancelling_pair, coeffs_for, expected_verdict, honest_base
from mixed_key_cases import NAMES, batch, mixed_keys, positions_of
from mixed_model import mixed_gt
from verify_cases import tamperings

import groth16_amd as g
from groth16_amd.binding import CURVE_ID, lib
from groth16_amd.verifier import (host_aggregate_gt, host_aggregate_mixed_gt, host_aggregate_mixed_verdict, host_aggregate_verdict,
                                  host_verdict)


@pytest.mark.parametrize("name", NAMES)
def test_one_key_equals_the_single_key_call(name):
    """n_keys = 1: both GT values byte-equal to g16_host_verify_aggregate_gt's, the verdict equal to g16_host_verify_aggregate's"""
    case = mixed_keys(name, 3)[1]
    cp = pm.CURVES[name]
    base = honest_base(name, case.vk, case.proofs, cp, extra=3)
    xs = [case.vectors[0]] * len(base)
    coeffs = coeffs_for(len(base), 4)
    lhs, rhs = host_aggregate_mixed_gt(name, [case.vk], [0] * len(base), base, xs, coeffs)
    want_lhs, want_rhs = host_aggregate_gt(name, case.vk, base, xs, coeffs)
    assert lhs.tobytes() == want_lhs.tobytes() and rhs.tobytes() == want_rhs.tobytes()
    assert (lhs == rhs).all()
    for label, proof, xi, want in tamperings(case.proofs, case.vectors[0], cp):
        flat, xt = [b.copy() for b in base], list(xs)
        flat[2], xt[2] = proof, xi
        assert host_aggregate_mixed_verdict(name, [case.vk], [0] * len(base), flat, xt, coeffs) \
            == host_aggregate_verdict(name, case.vk, flat, xt, coeffs) == expected_verdict([1] * (len(base) - 1) + [want]), label


@pytest.mark.parametrize("picks,key_of", [((0, 1), [1, 0, 1]), ((1, 2, 4), [2, 0, 1, 2, 0])], ids=["K2", "K3"])
@pytest.mark.parametrize("name", NAMES)
def test_both_sides_equal_the_model(name, picks, key_of):
    """two and three keys with their own trapdoors (and a derived one with another input count), keys interleaved"""
    keys = [mixed_keys(name, 7)[p] for p in picks]
    seen = [0] * len(keys)
    proofs, xs = [], []
    for k in key_of:
        proofs.append(keys[k].proofs[seen[k] % 2])
        xs.append(keys[k].vectors[seen[k] % len(keys[k].vectors)])
        seen[k] += 1
    coeffs = [3, (1 << 127) + 12345, 0xFEDCBA9876543210_0123456789ABCDEF, 1, (1 << 128) - 1][: len(key_of)]
    vks = [c.vk for c in keys]
    lhs, rhs = host_aggregate_mixed_gt(name, vks, key_of, proofs, xs, coeffs)
    want_lhs, want_rhs = mixed_gt(name, vks, key_of, proofs, xs, coeffs)
    assert (lhs == pmod.to_ark_limbs(name, want_lhs)).all()
    assert (rhs == pmod.to_ark_limbs(name, want_rhs)).all()
    assert (lhs == rhs).all()
    assert host_aggregate_mixed_verdict(name, vks, key_of, proofs, xs, coeffs) == 1


@pytest.mark.parametrize("name", NAMES)
def test_verdict_rule_over_the_tamperings(name):
    """1 if every proof's host_verdict under ITS key is 1, else 2 if any is 2, else 0 -- tamperings placed under each key in turn"""
    cp = pm.CURVES[name]
    keys = [mixed_keys(name, 7)[p] for p in (0, 2, 5)]   # 5: three public inputs
    vks = [c.vk for c in keys]
    flat0, key_of, xs0 = batch(keys, [2, 3, 2], order="shuffled", seed=5)
    n = len(key_of)
    assert host_aggregate_mixed_verdict(name, vks, key_of, flat0, xs0, coeffs_for(n, 1)) == 1
    assert host_aggregate_mixed_verdict(name, vks, key_of, flat0, xs0, None) == 1
    assert g.verify_proofs_aggregate_mixed_host(name, vks, key_of, flat0, xs0)
    count = 0
    for k, case in enumerate(keys):
        pos = positions_of(key_of, k)
        for t, (label, proof, xi, want) in enumerate(tamperings(case.proofs, case.vectors[0], cp)):
            if (t + k) % 3 and label != "wrong_input":   # a third of the set under each key, every tampering under some key
                continue
            flat, xt = flat0.copy(), list(xs0)
            i = pos[t % len(pos)]
            flat[i], xt[i] = proof, xi
            each = [host_verdict(name, vks[key_of[j]], flat[j], xt[j]) for j in range(n)]
            assert each[i] == want, (k, label)
            rule = expected_verdict(each)
            assert host_aggregate_mixed_verdict(name, vks, key_of, flat, xt, coeffs_for(n, 50 + count)) == rule, (k, label)
            if count % 4 == 0:
                assert host_aggregate_mixed_verdict(name, vks, key_of, flat, xt, None) == rule, (k, label)
            count += 1
    assert count >= 8


@pytest.mark.parametrize("name", NAMES)
def test_a_proof_under_the_wrong_key_is_rejected(name):
    keys = mixed_keys(name, 3)   # equal input counts, three trapdoors
    vks = [c.vk for c in keys]
    flat, key_of, xs = batch(keys, [2, 2, 1], order="round_robin")
    coeffs = coeffs_for(len(key_of), 9)
    assert host_aggregate_mixed_verdict(name, vks, key_of, flat, xs, coeffs) == 1
    for i in (0, len(key_of) - 1):
        wrong = key_of.copy()
        wrong[i] = (wrong[i] + 1) % 3
        assert host_aggregate_mixed_verdict(name, vks, wrong, flat, xs, coeffs) == 0
        assert host_aggregate_mixed_verdict(name, vks, wrong, flat, xs, None) == 0


@pytest.mark.parametrize("name", NAMES)
def test_sums_are_per_key(name):
    """cancelling_pair: C + D and C - D.  Both halves under ONE key, other keys' proofs between them: the plain product (all
    coefficients 1) accepts, because both reach the same S_C_k.  The halves under two DIFFERENT keys: D and -D meet different
    deltas and nothing cancels."""
    cp = pm.CURVES[name]
    keys = mixed_keys(name, 3)
    vks = [c.vk for c in keys]
    p2, q2 = cancelling_pair(keys[0].proofs[0], keys[0].proofs[1], cp)
    x = keys[0].vectors[0]
    flat = [p2, keys[1].proofs[0], keys[2].proofs[1], keys[1].proofs[1], q2]
    key_of, xs = [0, 1, 2, 1, 0], [x] * 5
    assert host_verdict(name, vks[0], p2, x) == 0 and host_verdict(name, vks[0], q2, x) == 0
    assert host_aggregate_mixed_verdict(name, vks, key_of, flat, xs, [1] * 5) == 1
    assert host_aggregate_mixed_verdict(name, vks, key_of, flat, xs, [1] * 4 + [2]) == 0
    assert host_aggregate_mixed_verdict(name, vks, key_of, flat, xs, coeffs_for(5, 3)) == 0
    # the same construction over two keys: a derived copy of key 0 takes the second half
    other = mixed_keys(name, 8)[7]
    assert other.num_public == keys[0].num_public
    p3, q3 = cancelling_pair(keys[0].proofs[0], other.proofs[1], cp)
    flat = [p3, keys[1].proofs[0], keys[2].proofs[1], keys[1].proofs[1], q3]
    assert host_aggregate_mixed_verdict(name, vks + [other.vk], [0, 1, 2, 1, 3], flat, xs, [1] * 5) == 0


@pytest.mark.parametrize("name", NAMES)
def test_empty_keys_repeated_keys_and_input_counts(name):
    keys = mixed_keys(name, 7)
    vks = [c.vk for c in keys]
    assert sorted(c.num_public for c in keys[3:]) == [0, 1, 3, 16]
    # keys 1 and 4 have no proof; 0 public inputs next to 16
    flat, key_of, xs = batch(keys, [1, 0, 2, 2, 0, 1, 2], order="shuffled", seed=2)
    coeffs = coeffs_for(len(key_of), 6)
    assert host_aggregate_mixed_verdict(name, vks, key_of, flat, xs, coeffs) == 1
    bad = list(xs)
    i = positions_of(key_of, 6)[1]
    bad[i] = bad[i].copy()
    bad[i][15, 0] ^= np.uint64(1)   # the last of the sixteen inputs of one proof
    assert host_aggregate_mixed_verdict(name, vks, key_of, flat, bad, coeffs) == 0
    # one key listed under two indices: the verdict of the batch does not change
    twice = key_of.copy()
    twice[positions_of(key_of, 2)[0]] = 7
    assert host_aggregate_mixed_verdict(name, vks + [vks[2]], twice, flat, xs, coeffs) == 1


@pytest.mark.parametrize("name", NAMES)
def test_errors_and_the_empty_batch(name):
    keys = mixed_keys(name, 3)
    vks = [c.vk for c in keys]
    cp = pm.CURVES[name]
    flat, key_of, xs = batch(keys, [1, 1, 1])
    assert host_aggregate_mixed_verdict(name, vks, [], np.zeros((0, 8 * cp.fq_limbs64), np.uint64), [], None) == 1
    assert host_aggregate_mixed_verdict(name, [], [], [], [], []) == 1

    def status(*args):
        with pytest.raises(g.G16Error) as err:
            host_aggregate_mixed_verdict(name, *args)
        return err.value

    assert status(vks, [0, 1, 3], flat, xs, [1, 2, 3]).status == 3          # key_of out of range
    assert status([], [0, 0, 0], flat, xs, [1, 2, 3]).status == 3           # proofs but no keys
    zero = status(vks, key_of, flat, xs, [1, 0, 3])                         # a zero coefficient
    assert zero.status == 3 and not isinstance(zero, g.SynthesisError)
    x = xs[0]
    assert isinstance(status(vks, key_of, flat, [np.concatenate([x, x[:1]])] + xs[1:], [1, 2, 3]), g.MalformedVerifyingKey)
    assert isinstance(status(vks, key_of, flat, [x[:0]] + xs[1:], None), g.MalformedVerifyingKey)
    with pytest.raises(g.MalformedVerifyingKey):   # n = 0 implies no inputs
        v = np.zeros(1, np.uint8)
        view, keep = vks[0].view()
        lib().check(lib().c.g16_host_verify_aggregate_mixed(CURVE_ID[name], C.byref(view), 1, None, None, 0, x.ctypes.data_as(C.POINTER(C.c_uint64)), 1,
                                                            None, v.ctypes.data_as(C.c_void_p)))
    with pytest.raises(ValueError):
        host_aggregate_mixed_verdict(name, vks, [0, 1], flat, xs, None)
    # a key view with a null member, an unknown curve, the _gt form without coefficients
    v = np.zeros(1, np.uint8)
    view, keep = vks[0].view()
    view.gamma_g2 = None
    ko = np.zeros(1, np.uint32)
    p64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    call = lib().c.g16_host_verify_aggregate_mixed
    one = np.ascontiguousarray(flat[0])
    xw = np.ascontiguousarray(x).reshape(-1)
    assert call(CURVE_ID[name], C.byref(view), 1, ko.ctypes.data_as(C.POINTER(C.c_uint32)), p64(one), 1, p64(xw), xw.size // 4, None,
                v.ctypes.data_as(C.c_void_p)) == 3
    view, keep = vks[0].view()
    assert call(7, C.byref(view), 1, ko.ctypes.data_as(C.POINTER(C.c_uint32)), p64(one), 1, p64(xw), xw.size // 4, None,
                v.ctypes.data_as(C.c_void_p)) == 3
    out = np.zeros(12 * cp.fq_limbs64, np.uint64)
    assert lib().c.g16_host_verify_aggregate_mixed_gt(CURVE_ID[name], C.byref(view), 1, ko.ctypes.data_as(C.POINTER(C.c_uint32)), p64(one), 1, p64(xw),
                                                      xw.size // 4, None, p64(out), p64(out)) == 3
