"""GPU tier: the verifier's input preparation in place -- the resident window tables of a prepared key (g16_dev_pvk_tables), one
prepare_inputs_tab per lane on them (g16_dev_prepare_inputs), and the verdict of every verifier path on proofs that are accepted
exactly when the device forms IC = gamma_abc_g1[0] + sum x_j gamma_abc_g1[j + 1] correctly -- against the host twins and pymodel's
big-integer group law, on the cases of tests/prepare_cases.py.  Affine Montgomery words are canonical: every comparison is bit for
bit, no tolerance anywhere."""
import numpy as np
import pytest

import pymodel as pm
import prepare_cases as pc
from helpers import g1_to_arr
from prepare_cases import FILL, N_KEYS, host_ic, host_tables, model_tables

import groth16_amd as g
from groth16_amd import binding as b
from groth16_amd.verifier import host_aggregate_mixed_verdict, host_aggregate_verdict, host_verdict, verify_batch_prepared

pytestmark = pytest.mark.gpu
NAMES = pc.NAMES
K = pc.source_constants()
BATCH_SIZES = sorted({v + e for v in (K["VERIFY_BLOCK"], K["AGG_SCALAR_BLOCK"], K["AGG_MAX_PER_LANE"]) for e in (-1, 0, 1)})


class Rig:
    """a prover of one curve and the prepared keys made on it, by crafted key"""

    def __init__(self, name, device=0):
        self.name = name
        self.prover = g.Groth16(name, device=device)
        self.pvks = {}
        self.host_verdicts = {}

    def pvk(self, key):
        if key not in self.pvks:
            self.pvks[key] = self.prover.prepare_verifying_key(key.vk)
        return self.pvks[key]

    def tables(self, key, device_index=0):
        return b.dev_pvk_tables(g.lib(), self.prover._ctx.handle, self.pvk(key).handle, key.num_public, b.FQ_LIMBS[self.name], device_index)

    def ic(self, key, rows_arr):
        st, out = b.dev_prepare_inputs(g.lib(), self.prover._ctx.handle, self.pvk(key).handle, rows_arr, key.num_public, b.FQ_LIMBS[self.name])
        assert st == 0
        return out

    def host_batch(self, key, proofs, rows_arr):
        """g16_host_verify per proof; a (proof, row) pair is verified once per module"""
        out = []
        for p, x in zip(proofs, rows_arr):
            tag = (key, p.tobytes(), x.tobytes())
            if tag not in self.host_verdicts:
                self.host_verdicts[tag] = host_verdict(self.name, key.vk, p, x)
            out.append(self.host_verdicts[tag])
        return out

    def close(self):
        for p in self.pvks.values():
            p.close()
        self.prover.close()


@pytest.fixture(scope="module", params=NAMES)
def rig(request):
    r = Rig(request.param)
    yield r
    r.close()


# ---- tables ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", range(3))
@pytest.mark.parametrize("num_public", [1, 5, 33])
def test_resident_tables_equal_host_and_model(rig, num_public, kind):
    """keys (a) random, (b) identity at gamma_abc_g1[0], (c) identity inside: every base against the host twin, and against the model
    every base (at 33 inputs: the first, the identity's neighbourhood and the last -- a wrong base stride shows at any j >= 1)"""
    key = pc.table_keys(rig.name, (num_public,))[kind]
    st, got = rig.tables(key)
    assert st == 0 and not (got == FILL).any()
    host = host_tables(key)
    bad = np.argwhere((got != host).any(axis=-1))
    assert bad.size == 0, (key, bad[:5].tolist())
    bases = list(range(num_public)) if num_public <= 5 else [0, 2, 17, 32]
    bad = np.argwhere((got[bases] != model_tables(key, bases)).any(axis=-1))
    assert bad.size == 0, (key, bases, bad[:5].tolist())
    for j, p in enumerate(key.points[1:]):
        assert (p is None) == (not got[j].any()), (key, j)


# ---- IC -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(N_KEYS))
def test_device_ic_equals_host_and_model(rig, idx):
    """batches of 1, 63, 64, 65 and 257 lanes, a different row in every lane: each wave mixes zero inputs, r - 1, the key's collision
    rows and ordinary rows"""
    key = pc.all_keys(rig.name)[idx]
    rows = pc.rows_for(key, 257)
    arr = pc.fr_rows(rig.name, rows)
    want = key.expected_ic_arr(rows)
    assert (host_ic(key, arr) == want).all(), key
    for n in (1, 63, 64, 65, 257):
        got = rig.ic(key, arr[:n])
        bad = np.flatnonzero((got != want[:n]).any(axis=1))
        assert bad.size == 0, (key, n, [(int(i), key.chain(rows[i])[:3]) for i in bad[:3]])
    # Groth16.prepare_inputs (the host route, variable-base) on the same rows
    for i in [0, 7, 14, 33][:2 if key.num_public > 5 else 4]:
        assert (rig.prover.prepare_inputs(rig.pvk(key), list(arr[i])).reshape(-1) == want[i]).all(), (key, i)


def test_every_lane_on_the_same_collision_row(rig):
    for key in pc.collision_keys(rig.name):
        for row, _ in key.collision_rows:
            got = rig.ic(key, pc.fr_rows(rig.name, [row] * 65))
            assert (got == key.expected_ic_arr([row])[0]).all(), (key, key.chain(row)[:2])


def test_device_lab_argument_checks(rig):
    lb, L = g.lib(), b.FQ_LIMBS[rig.name]
    key = pc.key_random(rig.name, 2)
    ctx, pvk = rig.prover._ctx.handle, rig.pvk(key).handle
    st, out = b.dev_prepare_inputs(lb, ctx, pvk, np.zeros((0, 2, 4), np.uint64), 2, L)
    assert st == 0 and out.shape == (0, 2 * L)
    st, out = b.dev_prepare_inputs(lb, ctx, pvk, pc.fr_rows(rig.name, [(1,)]), 1, L)
    assert st == 11 and (out == FILL).all()   # G16_ERR_MALFORMED_VK
    for index in (-1, 1):
        st, out = rig.tables(key, index)
        assert st == 3 and (out == FILL).all()   # G16_ERR_BAD_ARG: a single-device key has copy 0 only
    assert lb.c.g16_dev_prepare_inputs(None, pvk, None, 0, 0, None) == 3 and lb.c.g16_dev_pvk_tables(ctx, None, 0, None) == 3
    k0 = pc.key_random(rig.name, 0)
    assert (rig.ic(k0, np.zeros((3, 0, 4), np.uint64)) == g1_to_arr([k0.points[0]] * 3, k0.cp)).all()
    st, out = rig.tables(k0)
    assert st == 0 and out.size == 0


# ---- verdicts -------------------------------------------------------------------------------------------------------------------------
def device_verdicts(rig, key, proofs, rows):
    """(per-proof bytes of verify_verdicts, of verify_batch_prepared fed the device's IC, the aggregate verdict, the checked one)"""
    pv, pvk, flat = rig.prover, rig.pvk(key), np.stack(proofs)
    coeffs = pc.coefficients(len(proofs))
    ic = rig.ic(key, rows)
    return (list(pv.verify_verdicts(pvk, flat, rows)), list(verify_batch_prepared(pv._ctx, pvk, flat, ic)),
            pv.verify_aggregate_verdict(pvk, flat, rows, coeffs), pv.verify_aggregate_verdict(pvk, flat, rows, coeffs, check_subgroups=True))


@pytest.mark.parametrize("n", BATCH_SIZES)
@pytest.mark.parametrize("num_public", [0, 1, 5, 33])
def test_exact_verdicts_on_every_path(rig, num_public, n):
    """each honest batch gives 1; a single x_j + 1 at the first, a middle or the last position gives 0 (per proof: at that position
    alone); every result equals its host twin"""
    assert BATCH_SIZES == [3, 4, 5, 63, 64, 65, 255, 256, 257]
    key = pc.key_random(rig.name, num_public)
    coeffs = pc.coefficients(n)
    for pos in [None] + (pc.alter_positions(n) if num_public else []):
        proofs, rows = pc.verdict_batch(key, n, alter=pos)
        each = [int(i != pos) for i in range(n)]
        batch, prepared, agg, checked = device_verdicts(rig, key, proofs, rows)
        assert batch == each and prepared == each, (key, n, pos)
        assert agg == checked == int(pos is None), (key, n, pos, agg, checked)
        assert rig.host_batch(key, proofs, rows) == each, (key, n, pos)
        assert host_aggregate_verdict(rig.name, key.vk, proofs, rows, coeffs) == agg, (key, n, pos)


@pytest.mark.parametrize("idx", range(5, N_KEYS))
def test_exact_verdicts_on_the_crafted_keys(rig, idx):
    """keys (b) to (f): identity entries and the collision rows inside a batch of 65"""
    key = pc.all_keys(rig.name)[idx]
    n = K["VERIFY_BLOCK"] + 1
    coeffs = pc.coefficients(n)
    for pos in (None, 0, 7, n - 1):   # rows 0 and 7 are collision rows where the key has them
        proofs, rows = pc.verdict_batch(key, n, alter=pos)
        each = [int(i != pos) for i in range(n)]
        batch, prepared, agg, checked = device_verdicts(rig, key, proofs, rows)
        assert batch == each and prepared == each, (key, pos)
        assert agg == checked == int(pos is None), (key, pos)
        assert rig.host_batch(key, proofs, rows) == each and host_aggregate_verdict(rig.name, key.vk, proofs, rows, coeffs) == agg, (key, pos)


@pytest.mark.parametrize("n", BATCH_SIZES)
@pytest.mark.parametrize("pair", [(5, 1), (33, 0)])
def test_exact_verdicts_mixed_keys(rig, pair, n):
    """two keys with different input counts, interleaved proof by proof"""
    keys = [pc.key_random(rig.name, m) for m in pair]
    pvks = [rig.pvk(k) for k in keys]
    coeffs = pc.coefficients(n)
    for pos in [None] + pc.alter_positions(n):
        if pos is not None and not keys[pos % 2].num_public:
            pos -= 1   # that proof's key takes no input: alter its neighbour
        key_of, proofs, rows = pc.mixed_batch(keys, n, alter=pos)
        got = rig.prover.verify_aggregate_mixed_verdict(pvks, key_of, np.stack(proofs), rows, coeffs)
        assert got == int(pos is None), (pair, n, pos)
        assert rig.prover.verify_aggregate_mixed_verdict(pvks, key_of, np.stack(proofs), rows, coeffs, check_subgroups=True) == got
        assert host_aggregate_mixed_verdict(rig.name, [k.vk for k in keys], key_of, proofs, rows, coeffs) == got, (pair, n, pos)


def test_collision_rows_of_eight_keys_in_one_mixed_batch(rig):
    keys = pc.collision_keys(rig.name)
    pvks = [rig.pvk(k) for k in keys]
    key_of = list(range(len(keys)))
    rows = [k.collision_rows[0][0] for k in keys]
    proofs = np.stack([k.proof(row, i) for i, (k, row) in enumerate(zip(keys, rows))])
    xs = [pc.fr_rows(rig.name, [row])[0] for row in rows]
    coeffs = pc.coefficients(len(keys))
    assert rig.prover.verify_aggregate_mixed_verdict(pvks, key_of, proofs, xs, coeffs) == 1
    for pos in (0, 3, 7):
        bad = list(xs)
        bad[pos] = pc.fr_rows(rig.name, [pc.bump(rows[pos], 0, pm.CURVES[rig.name].r)])[0]
        assert rig.prover.verify_aggregate_mixed_verdict(pvks, key_of, proofs, bad, coeffs) == 0, pos


# ---- two devices ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_two_device_context_tables_of_both_copies_and_a_verdict_batch(name):
    multi = Rig(name, device=[0, 0])
    try:
        key = pc.key_identity_inside(name)
        host = host_tables(key)
        for index in (0, 1):
            st, got = multi.tables(key, index)
            assert st == 0 and (got == host).all(), index
        st, out = multi.tables(key, 2)
        assert st == 3 and (out == FILL).all()
        n = K["VERIFY_BLOCK"] + 1   # 32 proofs on one copy, 33 on the other
        for pos in (None, 0, n // 2, n - 1):
            proofs, rows = pc.verdict_batch(key, n, alter=pos)
            each = [int(i != pos) for i in range(n)]
            batch, prepared, agg, checked = device_verdicts(multi, key, proofs, rows)
            assert batch == each and prepared == each and agg == checked == int(pos is None), pos
    finally:
        multi.close()


# ---- unreduced input words ------------------------------------------------------------------------------------------------------------
def test_every_path_reads_an_unreduced_row_as_its_residue(rig):
    """Rows whose words are x + r, and one of all-ones words.  The entry points take raw Montgomery words and do not check them
    against r; to_canonical reduces, so the table walk sees x mod r, and the aggregate forms multiply the raw words by a reduced
    coefficient, which leaves a fully reduced product.  Pinned: the device's IC and its host twin equal the model at the reduced
    value, and batch, prepared, aggregate, checked aggregate and mixed -- device and host -- give ONE verdict per case, the model's
    at that value (1 for proofs made for it, 0 for proofs made for the value + 1).  They agree, so x and x + r are one input
    (include/g16_mi355x.h says so beside g16_verify_batch)."""
    name = rig.name
    key, rows, reduced, honest, wrong = pc.unreduced_case(name)
    n = len(reduced)
    want_ic = key.expected_ic_arr([(v,) for v in reduced])
    assert (rig.ic(key, rows) == want_ic).all() and (host_ic(key, rows) == want_ic).all()
    coeffs = pc.coefficients(n)
    pvk = rig.pvk(key)
    for proofs, want in ((honest, 1), (wrong, 0)):
        seen = {"host batch": rig.host_batch(key, proofs, rows), "host aggregate": host_aggregate_verdict(name, key.vk, proofs, rows, coeffs),
                "host mixed": host_aggregate_mixed_verdict(name, [key.vk, key.vk], [i % 2 for i in range(n)], proofs, list(rows), coeffs)}
        seen["batch"], seen["prepared"], seen["aggregate"], seen["checked"] = device_verdicts(rig, key, proofs, rows)
        seen["mixed"] = rig.prover.verify_aggregate_mixed_verdict([pvk, pvk], [i % 2 for i in range(n)], np.stack(proofs), list(rows), coeffs)
        for i in range(n):   # row by row through the aggregate forms: one wrong row cannot hide behind the others
            seen["aggregate row %d" % i] = rig.prover.verify_aggregate_verdict(pvk, np.stack(proofs[i:i + 1]), rows[i:i + 1], coeffs[:1])
            seen["mixed row %d" % i] = rig.prover.verify_aggregate_mixed_verdict([pvk], [0], np.stack(proofs[i:i + 1]), [rows[i]], coeffs[:1])
        print(name, "proofs made for the reduced value" if want else "proofs made for the reduced value + 1", seen)
        assert all(v == want or v == [want] * n for v in seen.values()), (want, seen)
