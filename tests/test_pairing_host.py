"""CPU tier: the optimal-ate pairing and the verifier of groth16_amd on the host (g16_host_pairing / g16_host_verify run the same
pairing.hpp templates as the GPU kernels) against the big-int model of tests/pairing_model.py and pymodel's Groth16 verifier."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pairing_model as pmod
import pymodel as pm
from helpers import g1_to_arr, g2_to_arr
from verify_cases import identity_ic_case, nonsubgroup_pairs_with_model, oracle_case, pm_proof, pm_vk, pymodel_case, tamperings, torsion_pair

import groth16_amd as g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["bls12_381", "bn254"]


@pytest.mark.parametrize("name", NAMES)
def test_model_order_nondegeneracy_and_identity(name):
    cp = pm.CURVES[name]
    F = pm.Fq12(cp)
    e = pmod.pairing(name, cp.g1, cp.g2)
    assert e != F.one
    assert F.pow(e, cp.r) == F.one
    assert pmod.pairing(name, None, cp.g2) == F.one
    assert pmod.pairing(name, cp.g1, None) == F.one


@pytest.mark.parametrize("name", NAMES)
def test_model_bilinearity(name):
    cp = pm.CURVES[name]
    G1, G2 = pm.groups(cp)
    F = pm.Fq12(cp)
    a, b = 0x1234567, 0x89ABCDE
    e = pmod.pairing(name, cp.g1, cp.g2)
    assert pmod.pairing(name, G1.mul(cp.g1, a), G2.mul(cp.g2, b)) == F.pow(e, a * b)


@pytest.mark.parametrize("name", NAMES)
def test_host_pairing_equals_model(name):
    cp = pm.CURVES[name]
    G1, G2 = pm.groups(cp)
    P2, Q3 = G1.mul(cp.g1, 0xDEADBEEF12345), G2.mul(cp.g2, 0x7777777777)
    cases = [[(cp.g1, cp.g2)], [(P2, cp.g2)], [(cp.g1, Q3)], [(None, cp.g2)], [(cp.g1, None)], [(P2, Q3), (cp.g1, cp.g2)],
             [(P2, cp.g2), (None, Q3), (G1.neg(cp.g1), Q3)]]
    for pairs in cases:
        want = pmod.to_ark_limbs(name, pmod.pairing_product(name, pairs))
        got = g.host_pairing(name, g1_to_arr([p for p, _ in pairs], cp), g2_to_arr([q for _, q in pairs], cp))
        assert (got == want).all(), pairs


@pytest.mark.parametrize("name", NAMES)
def test_host_pairing_of_nothing_is_one(name):
    cp = pm.CURVES[name]
    got = g.host_pairing(name, np.zeros((0, 2 * cp.fq_limbs64), np.uint64), np.zeros((0, 4 * cp.fq_limbs64), np.uint64))
    assert (got == pmod.to_ark_limbs(name, pm.Fq12(cp).one)).all()


@pytest.mark.parametrize("name", NAMES)
def test_host_pairing_outside_the_subgroups_equals_model(name):
    """the plain verifier accepts any on-curve B: the Miller loop on S + T_l (and on BLS12-381 a G1 point outside its subgroup)"""
    cp = pm.CURVES[name]
    for label, pairs, want in nonsubgroup_pairs_with_model(name):
        got = g.host_pairing(name, g1_to_arr([p for p, _ in pairs], cp), g2_to_arr([q for _, q in pairs], cp))
        assert (got == want).all(), label


def pairing_outcome(call):
    """the GT limbs, or the exception's type where the entry point reports a status"""
    try:
        return list(call())
    except g.G16Error as e:
        return type(e)


@pytest.mark.parametrize("name", NAMES)
def test_host_pairing_of_a_pure_torsion_point_is_deterministic(name):
    """Q = T_l alone: on BLS12-381 (l = 13) the chain of multiples reaches [13 k] Q, the projective T passes through z = 0 and the
    loop value becomes 0, which the entry point reports as an unexpected identity.  The big-int model works on affine points and
    defines no value there, so this pins the outcome only: the same on every call (tests/test_gpu_verify.py: and on the GPU)."""
    cp = pm.CURVES[name]
    l, P, T, hits = torsion_pair(name)
    assert hits == (name == "bls12_381")
    a, b = g1_to_arr([P], cp), g2_to_arr([T], cp)
    first = pairing_outcome(lambda: g.host_pairing(name, a, b))
    assert first == pairing_outcome(lambda: g.host_pairing(name, a, b))
    if hits:
        assert first is g.UnexpectedIdentity


@pytest.mark.parametrize("name", NAMES)
def test_host_cancelling_pairs_give_the_unit(name):
    cp = pm.CURVES[name]
    G1, G2 = pm.groups(cp)
    P, Q = G1.mul(cp.g1, 0x5EED), G2.mul(cp.g2, 0xF00D)
    got = g.host_pairing(name, g1_to_arr([P, G1.neg(P)], cp), g2_to_arr([Q, Q], cp))
    assert (got == pmod.to_ark_limbs(name, pm.Fq12(cp).one)).all()
    got = g.host_pairing(name, g1_to_arr([P, P], cp), g2_to_arr([Q, G2.neg(Q)], cp))
    assert (got == pmod.to_ark_limbs(name, pm.Fq12(cp).one)).all()


@pytest.mark.parametrize("name", NAMES)
def test_host_verify_with_identity_ic(name):
    """gamma_abc_g1 = [-k G, G] and the input k: the prepared input is the identity and its pair contributes nothing"""
    vk, proofs, x_good, x_bad, cp = identity_ic_case(name)
    for p in proofs:
        assert g.verifier.host_verdict(name, vk, p, x_good) == 1
        assert g.verifier.host_verdict(name, vk, p, x_bad) == 0
    assert g.verifier.host_aggregate_verdict(name, vk, proofs, [x_good] * len(proofs)) == 1
    assert g.verifier.host_aggregate_verdict(name, vk, proofs, [x_good, x_bad] + [x_good] * (len(proofs) - 2)) == 0


@pytest.mark.parametrize("make", [oracle_case, pymodel_case], ids=["oracle_syn", "pymodel_mimc"])
@pytest.mark.parametrize("name", NAMES)
def test_host_verify_matches_pymodel(name, make):
    vk, proofs, x, cp = make(name)
    pvk = pm_vk(vk, cp)
    from helpers import mont_to_ints
    for label, proof, xs, want in tamperings(proofs, x, cp):
        got = g.verifier.host_verdict(name, vk, proof, xs)
        assert got == want, label
        if want != 2 and label in ("honest", "wrong_input", "c_is_a", "b_other", "a_neg"):
            assert pm.verify_proof(cp, pvk, pm_proof(proof, cp), mont_to_ints(xs.reshape(-1, 4), cp.r)) == (want == 1), label
        assert g.verify_proof_host(name, vk, proof, xs) == (want == 1)


@pytest.mark.parametrize("name", NAMES)
def test_host_verify_wrong_input_length_is_malformed_vk(name):
    vk, proofs, x, cp = oracle_case(name)
    with pytest.raises(g.MalformedVerifyingKey):
        g.verify_proof_host(name, vk, proofs[0], np.concatenate([x, x[:1]]))
    with pytest.raises(g.MalformedVerifyingKey):
        g.verify_proof_host(name, vk, proofs[0], x[:0])


def test_vk_view_struct_size_and_status():
    lb = g.lib()
    assert lb.c.g16_struct_size(6) == C.sizeof(g.binding.VkViewC) == 48
    assert lb.c.g16_strerror(11).decode().startswith("malformed verifying key")


def test_verifying_key_from_proving_key_needs_gamma():
    cp = pm.BLS12_381
    z = np.zeros((1, 12), np.uint64)
    pk = g.ProvingKey("bls12_381", z, z, z, np.zeros((1, 24), np.uint64), np.zeros((1, 24), np.uint64), z, z, z, z, z)
    with pytest.raises(ValueError):
        g.VerifyingKey.from_proving_key(pk)
    pk.gamma_g2, pk.gamma_abc_g1 = np.zeros((1, 24), np.uint64), np.zeros((3, 12), np.uint64)
    assert g.VerifyingKey.from_proving_key(pk).num_public == 2


def test_c99_consumer_of_the_verify_entry_points(tmp_path):
    """built as tests/test_abi_consumer.py builds its program"""
    exe = str(tmp_path / "abi_verify")
    libdir = os.path.join(ROOT, "groth16_amd")
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "abi_verify.c"), "-o", exe, "-L", libdir, "-l:libg16_mi355x.so", f"-Wl,-rpath,{libdir}"]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert "abi_verify ok" in run.stdout
