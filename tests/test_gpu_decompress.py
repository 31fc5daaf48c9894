"""GPU tier: the decompression kernels (verify_decompress.hip) against the host twin and the case list, per point and per proof,
and g16_verify_aggregate_bytes -- bytes to verdict -- against the checked aggregate verifier on the decoded proofs, on both curves."""
import numpy as np
import pytest

from aggregate_cases import coeffs_for, honest_base
from decompress_cases import NAMES, blob, cases, enc_size, fq_bytes, proofs_to_bytes
from helpers import arr_to_g2, g2_to_arr
from subgroup_cases import cases as subgroup_cases
from subgroup_cases import model_groups
from verify_cases import oracle_case, wrong_input

import groth16_amd as g
from groth16_amd.verifier import host_aggregate_verdict

pytestmark = pytest.mark.gpu
N_PROOFS = 67


@pytest.fixture(scope="module", params=NAMES)
def setup(request):
    name = request.param
    vk, proofs, x, cp = oracle_case(name)
    base = honest_base(name, vk, proofs, cp)
    honest = np.stack([base[i % len(base)] for i in range(N_PROOFS)])
    with g.Groth16(name, device=0) as prover:
        pvk = prover.prepare_verifying_key(vk)
        yield name, prover, pvk, vk, x, cp, honest
        pvk.close()


def invalid_encoding(name, g2, label):
    labels, encs, status, _ = cases(name, g2)
    i = labels.index(label)
    assert status[i] == 0
    return np.frombuffer(encs[i], dtype=np.uint8)


def corrupted(name, data):
    """(bytes, status, where): A, B and C of three separate proofs replaced by three different kinds of invalid encoding"""
    fb = fq_bytes(name)
    out, want = data.copy(), np.ones(N_PROOFS, dtype=np.uint8)
    where = {3: (0, fb, False, "no_point"), 20: (fb, 3 * fb, True, "c1_eq_p"), 40: (3 * fb, 4 * fb, False, "infinity_and_sign")}
    for i, (lo, hi, g2, label) in where.items():
        out[i, lo:hi] = invalid_encoding(name, g2, label)
        want[i] = 0
    return out, want, where


def b_plus_torsion(flat, cp, name):
    """the proof with B replaced by B + T, T of the smallest prime order outside the subgroup: on its curve, not a member"""
    L = cp.fq_limbs64
    G = model_groups(cp)[1]
    _, torsion = subgroup_cases(name, True)
    out = flat.copy()
    out[2 * L: 6 * L] = g2_to_arr([G.add(arr_to_g2(flat[2 * L: 6 * L], cp)[0], torsion[min(torsion)])], cp)[0]
    return out


@pytest.mark.parametrize("g2", [False, True])
def test_points_equal_the_host_twin(setup, g2):
    """the whole case list tiled to 130 points: two full waves and a 2-lane tail"""
    name, prover = setup[0], setup[1]
    labels, encs, status, pts = cases(name, g2)
    idx = np.arange(130) % len(labels)
    data = blob(encs, idx)
    got, st = prover.decompress_points(data, g2)
    host, host_st = g.decompress_points_host(name, data, g2)
    print(name, "g2" if g2 else "g1", "device status", st[: len(labels)].tolist(), "cases", status.tolist())
    assert st.tobytes() == host_st.tobytes() and (st == status[idx]).all()
    assert got.tobytes() == host.tobytes() == np.ascontiguousarray(pts[idx]).tobytes()
    empty, est = prover.decompress_points(b"", g2)
    assert empty.shape[0] == 0 and est.shape == (0,)
    with pytest.raises(ValueError):
        prover.decompress_points(data[:-1], g2)


def check_proofs(prover, name, honest):
    data = proofs_to_bytes(name, honest)
    flat, st = prover.decompress_proofs(data)
    assert (st == 1).all() and flat.tobytes() == honest.tobytes()
    bad, want, where = corrupted(name, data)
    flat, st = prover.decompress_proofs(bad.tobytes())
    print(name, "proof status", st.tolist())
    assert (st == want).all()
    keep = want == 1
    assert flat[keep].tobytes() == honest[keep].tobytes()
    L = honest.shape[1] // 8
    for i, (lo, hi, g2, _) in where.items():   # the undecodable point is the identity, its neighbours are decoded
        wlo, whi = {0: (0, 2 * L), fq_bytes(name): (2 * L, 6 * L)}.get(lo, (6 * L, 8 * L))
        expect = honest[i].copy()
        expect[wlo:whi] = 0
        assert flat[i].tobytes() == expect.tobytes(), i
    empty, est = prover.decompress_proofs(b"")
    assert empty.shape == (0, 8 * L) and est.shape == (0,)
    with pytest.raises(ValueError):
        prover.decompress_proofs(data.tobytes()[:-enc_size(name, False)])


def test_proofs(setup):
    name, prover, pvk, vk, x, cp, honest = setup
    check_proofs(prover, name, honest)


def test_proofs_on_two_chunks(setup):
    """a context listing the one GPU twice cuts the batch into two chunks: the order survives the split"""
    name, honest = setup[0], setup[6]
    with g.Groth16(name, device=[0, 0]) as multi:
        check_proofs(multi, name, honest)
        _, encs, status, pts = cases(name, True)
        got, st = multi.decompress_points(blob(encs), True)
        assert (st == status).all() and got.tobytes() == pts.tobytes()
        # n = 1: the first of the two chunks is empty.  One honest and one corrupted item, against the host twin
        fb = fq_bytes(name)
        data = proofs_to_bytes(name, honest)
        bad, want, _ = corrupted(name, data)
        for row, ok in ((data[0], 1), (bad[3], 0)):
            parts = [g.decompress_points_host(name, row[lo:hi], g2) for lo, hi, g2 in ((0, fb, False), (fb, 3 * fb, True), (3 * fb, 4 * fb, False))]
            flat, st = multi.decompress_proofs(row)
            assert flat.tobytes() == b"".join(p.tobytes() for p, _ in parts)
            assert list(st) == [min(int(s[0]) for _, s in parts)] == [ok]
        for i in (int(np.argmax(status == 1)), int(np.argmax(status == 0))):
            got, st = multi.decompress_points(blob(encs, [i]), True)
            host, host_st = g.decompress_points_host(name, blob(encs, [i]), True)
            assert got.tobytes() == host.tobytes() and list(st) == list(host_st) == [status[i]]


def test_bytes_to_verdict(setup):
    name, prover, pvk, vk, x, cp, honest = setup
    xs = [x] * N_PROOFS
    coeffs = coeffs_for(N_PROOFS, 11)
    data = proofs_to_bytes(name, honest)
    decoded, _ = prover.decompress_proofs(data)
    assert prover.verify_aggregate_bytes_verdict(pvk, data, xs, coeffs) == 1
    assert prover.verify_aggregate_verdict(pvk, decoded, xs, coeffs, check_subgroups=True) == 1
    assert prover.verify_proofs_aggregate_bytes(pvk, data.tobytes(), xs) is True   # coefficients from the operating system
    bad_x = list(xs)
    bad_x[66] = wrong_input(x, cp)
    assert prover.verify_aggregate_bytes_verdict(pvk, data, bad_x, coeffs) == 0
    outside = honest.copy()
    outside[31] = b_plus_torsion(outside[31], cp, name)
    outside_bytes = proofs_to_bytes(name, outside)
    assert prover.verify_aggregate_bytes_verdict(pvk, outside_bytes, xs, coeffs) == 3
    assert prover.verify_aggregate_verdict(pvk, prover.decompress_proofs(outside_bytes)[0], xs, coeffs, check_subgroups=True) == 3
    both, _, _ = corrupted(name, outside_bytes)   # undecodable proofs and the torsion proof in one batch: 4 wins
    assert prover.verify_aggregate_bytes_verdict(pvk, both, xs, coeffs) == 4
    assert prover.verify_proofs_aggregate_bytes(pvk, both, xs, coeffs) is False
    assert prover.verify_aggregate_bytes_verdict(pvk, b"", [], None) == 1
    with pytest.raises(ValueError):
        prover.verify_aggregate_bytes_verdict(pvk, data.tobytes()[:-1], xs, coeffs)
    with pytest.raises(ValueError):
        prover.verify_aggregate_bytes_verdict(pvk, data, xs[:-1], coeffs)
    with pytest.raises(g.G16Error):   # a zero coefficient would drop its proof out of the check
        prover.verify_aggregate_bytes_verdict(pvk, data, xs, [0] + coeffs[1:])
    with pytest.raises(g.MalformedVerifyingKey):
        prover.verify_aggregate_bytes_verdict(pvk, data, [np.concatenate([x, x])] * N_PROOFS, coeffs)
    with g.Groth16(name, device=[0, 0]) as multi:   # each device decodes and checks its own chunk
        pvk2 = multi.prepare_verifying_key(vk)
        try:
            for d, xt, want in ((data, xs, 1), (data, bad_x, 0), (outside_bytes, xs, 3), (both, xs, 4)):
                assert multi.verify_aggregate_bytes_verdict(pvk2, d, xt, coeffs) == want
            # n = 1: the first of the two chunks is empty
            for i, xt, want in ((0, xs[:1], 1), (66, bad_x[66:], 0)):
                assert multi.verify_aggregate_bytes_verdict(pvk2, data[i], xt, coeffs[:1]) == want
                assert host_aggregate_verdict(name, vk, honest[i: i + 1], xt, coeffs[:1]) == want
        finally:
            pvk2.close()
