"""CPU tier: the verifier's input preparation on the host twins (g16_host_pvk_tables / g16_host_prepare_inputs run the table
kernel's entry function and the kernels' prepare_inputs_tab compiled for the host) against pymodel's big-integer group law, on the
cases of tests/prepare_cases.py: every table entry, the edge scalars, identity entries in the key, doubling / cancelling table
additions, an identity IC; and the exact-verdict proofs through g16_host_verify, g16_host_verify_aggregate and
g16_host_verify_aggregate_mixed.  Affine Montgomery words are canonical: every comparison is bit for bit."""
import types

import numpy as np
import pytest

import pymodel as pm
import prepare_cases as pc
from helpers import g1_to_arr

import groth16_amd as g
from groth16_amd import binding as b

NAMES = pc.NAMES
FILL, N_KEYS = pc.FILL, pc.N_KEYS
host_tables, host_ic, model_tables = pc.host_tables, pc.host_ic, pc.model_tables


@pytest.mark.parametrize("kind", range(3))
@pytest.mark.parametrize("num_public", [1, 5])
@pytest.mark.parametrize("name", NAMES)
def test_host_tables_equal_the_model_at_every_entry(name, num_public, kind):
    key = pc.table_keys(name, (num_public,))[kind]
    got = host_tables(key)
    assert not (got == FILL).any(), key
    want = model_tables(key)
    bad = np.argwhere((got != want).any(axis=-1))
    assert bad.size == 0, (key, bad[:5].tolist())   # (base, window, digit - 1) of the first wrong entries
    for j, p in enumerate(key.points[1:]):
        assert (p is None) == (not got[j].any()), (key, j)   # an identity base: 960 identity entries, and nowhere else


@pytest.mark.parametrize("idx", range(N_KEYS))
@pytest.mark.parametrize("name", NAMES)
def test_host_prepare_inputs_equals_the_model_on_every_key(name, idx):
    assert len(pc.all_keys(name)) == N_KEYS
    key = pc.all_keys(name)[idx]
    n = max(len(pc.scalar_list(name)) + 8, 65) if key.num_public else 2
    rows = pc.rows_for(key, n)
    got = host_ic(key, pc.fr_rows(name, rows))
    want = key.expected_ic_arr(rows)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (key, [(int(i), key.chain(rows[i])[:3]) for i in bad[:3]])
    if key.num_public == 1:   # the whole scalar list went through the one input
        assert {row[0] for row in rows} >= set(pc.scalar_list(name))


@pytest.mark.parametrize("name", NAMES)
def test_host_identity_ic_leaves_as_all_zero_words(name):
    f = pc.key_identity_ic(name)
    assert not host_ic(f, pc.fr_rows(name, [f.collision_rows[0][0]])).any()


@pytest.mark.parametrize("name", NAMES)
def test_host_prepare_inputs_every_lane_on_one_collision_row(name):
    for key in pc.collision_keys(name):
        for row, _ in key.collision_rows:
            got = host_ic(key, pc.fr_rows(name, [row] * 3))
            assert (got == key.expected_ic_arr([row])[0]).all(), (key, key.chain(row)[:2])


@pytest.mark.parametrize("name", NAMES)
def test_host_lab_argument_checks(name):
    lb, cid, L = g.lib(), b.CURVE_ID[name], b.FQ_LIMBS[name]
    key = pc.key_random(name, 2)
    view, keep = key.vk.view()
    st, out = b.host_prepare_inputs(lb, cid, view, np.zeros((0, 2, 4), np.uint64), 2, L)
    assert st == 0 and out.shape == (0, 2 * L)
    st, out = b.host_prepare_inputs(lb, cid, view, pc.fr_rows(name, [(1,)]), 1, L)
    assert st == 11 and (out == FILL).all()   # G16_ERR_MALFORMED_VK, nothing written
    st, out = b.host_prepare_inputs(lb, 7, view, pc.fr_rows(name, [(1, 2)]), 2, L)
    assert st != 0 and (out == FILL).all()
    assert lb.c.g16_host_pvk_tables(cid, None, None) != 0
    k0 = pc.key_random(name, 0)
    v0, keep0 = k0.vk.view()
    assert lb.c.g16_host_pvk_tables(cid, v0, None) == 0   # no base, no table
    assert (host_ic(k0, np.zeros((2, 0, 4), np.uint64)) == g1_to_arr([k0.points[0]] * 2, k0.cp)).all()


@pytest.mark.parametrize("name", NAMES)
def test_groth16_prepare_inputs_host_route_equals_the_model(name):
    """Groth16.prepare_inputs (variable-base multiplications through g16_host_group_op) on the same rows; it needs no context, so
    it is called on a stand-in that carries the curve and the library"""
    me = types.SimpleNamespace(curve=name, _ctx=types.SimpleNamespace(lib=g.lib()))
    r = pm.CURVES[name].r
    keys = [pc.key_random(name, 0), pc.key_random(name, 2), pc.key_identity_first(name), pc.key_identity_inside(name)] + pc.collision_keys(name)
    for key in keys:
        rows = [row for row, _ in key.collision_rows] + pc.rows_for(key, 8)[1:4]
        if key.num_public == 2:
            rows += [(0, 0), (r - 1, 1), (1, r - 1)]
        for row in rows:
            got = g.Groth16.prepare_inputs(me, key.vk, list(pc.fr_rows(name, [row])[0]))
            assert (got == key.expected_ic_arr([row])[0]).all(), (key, row)
    with pytest.raises(g.MalformedVerifyingKey):
        g.Groth16.prepare_inputs(me, pc.key_random(name, 2).vk, list(pc.fr_rows(name, [(1,)])[0]))


def host_verdicts(key, proofs, rows_arr):
    return [g.verifier.host_verdict(key.curve, key.vk, p, x) for p, x in zip(proofs, rows_arr)]


@pytest.mark.parametrize("name", NAMES)
def test_host_verdicts_are_exact_on_every_key(name):
    """a proof made for ic = g_0 + sum x_j g_j is accepted exactly when the verifier forms that IC; with one x_j + 1 it is rejected"""
    n = pc.source_constants()["AGG_MAX_PER_LANE"] + 1
    coeffs = pc.coefficients(n)
    for key in pc.all_keys(name):
        proofs, rows = pc.verdict_batch(key, n)
        assert host_verdicts(key, proofs, rows) == [1] * n, key
        assert g.verifier.host_aggregate_verdict(name, key.vk, proofs, rows, coeffs) == 1, key
        if not key.num_public:
            continue
        for pos in pc.alter_positions(n):
            proofs, rows = pc.verdict_batch(key, n, alter=pos)
            assert host_verdicts(key, proofs, rows) == [int(i != pos) for i in range(n)], (key, pos)
            assert g.verifier.host_aggregate_verdict(name, key.vk, proofs, rows, coeffs) == 0, (key, pos)


@pytest.mark.parametrize("name", NAMES)
def test_host_verdicts_with_eight_collision_rows_in_one_batch(name):
    """every proof of the batch on a collision row of its own key is not possible under one key; the mixed form takes them all"""
    keys = pc.collision_keys(name)
    key_of = list(range(len(keys)))
    rows = [k.collision_rows[0][0] for k in keys]
    proofs = [k.proof(row, i) for i, (k, row) in enumerate(zip(keys, rows))]
    xs = [pc.fr_rows(name, [row])[0] for row in rows]
    coeffs = pc.coefficients(len(keys))
    assert g.verifier.host_aggregate_mixed_verdict(name, [k.vk for k in keys], key_of, proofs, xs, coeffs) == 1
    for pos in (0, 3, 7):
        bad = list(xs)
        bad[pos] = pc.fr_rows(name, [pc.bump(rows[pos], 0, pm.CURVES[name].r)])[0]
        assert g.verifier.host_aggregate_mixed_verdict(name, [k.vk for k in keys], key_of, proofs, bad, coeffs) == 0, pos


@pytest.mark.parametrize("name", NAMES)
def test_host_mixed_verdicts_two_keys_interleaved(name):
    keys = [pc.key_random(name, 5), pc.key_equal_bases(name), pc.key_random(name, 1)]   # 5, 5 and 1 inputs
    vks = [k.vk for k in keys]
    n = 2 * pc.source_constants()["AGG_MAX_PER_LANE"] + 1
    coeffs = pc.coefficients(n)
    key_of, proofs, rows = pc.mixed_batch(keys, n)
    assert g.verifier.host_aggregate_mixed_verdict(name, vks, key_of, proofs, rows, coeffs) == 1
    for pos in pc.alter_positions(n):
        key_of, proofs, rows = pc.mixed_batch(keys, n, alter=pos)
        assert g.verifier.host_aggregate_mixed_verdict(name, vks, key_of, proofs, rows, coeffs) == 0, pos


@pytest.mark.parametrize("name", NAMES)
def test_host_paths_read_an_unreduced_row_as_its_residue(name):
    """Rows whose words are x + r (one all-ones): to_canonical reduces, so the table walk sees x mod r; the aggregate forms multiply
    the raw words by a reduced coefficient, and a Montgomery product with one operand below r is fully reduced whatever the other
    holds.  All host paths must therefore agree with the model at the reduced value."""
    key, rows, reduced, honest, wrong = pc.unreduced_case(name)
    n = len(reduced)
    assert (host_ic(key, rows) == key.expected_ic_arr([(v,) for v in reduced])).all()
    coeffs = pc.coefficients(n)
    for proofs, want in ((honest, 1), (wrong, 0)):
        assert host_verdicts(key, proofs, rows) == [want] * n
        assert g.verifier.host_aggregate_verdict(name, key.vk, proofs, rows, coeffs) == want
        assert g.verifier.host_aggregate_mixed_verdict(name, [key.vk, key.vk], [i % 2 for i in range(n)], proofs, list(rows), coeffs) == want
        for i in range(n):   # row by row as well: one wrong row cannot hide behind the others
            assert g.verifier.host_aggregate_verdict(name, key.vk, proofs[i:i + 1], rows[i:i + 1], coeffs[:1]) == want, i
