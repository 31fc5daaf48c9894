"""CPU tier: the premises of tests/prepare_cases.py, pinned by model arithmetic alone (pymodel's big-integer group law): the scalar
list reaches every table entry a canonical scalar can select, the crafted keys really produce the collisions they are named for on
the chain of partial sums prepare_inputs_tab forms, and the exact-verdict proofs satisfy the Groth16 equation in the exponent."""
import pytest

import pymodel as pm
import prepare_cases as pc

NAMES = pc.NAMES


def test_the_sources_spell_the_order_the_cases_are_derived_for():
    """chain() replays bases in order and windows from 0 upward.  If prepare_inputs_tab or tab_accumulate is reordered, the
    collisions below no longer happen where the cases put them: re-derive the cases, then update loop_order_in_source."""
    assert pc.loop_order_in_source() == (True, True)
    k = pc.source_constants()
    assert (k["WINDOWS"], k["DIGITS"]) == (pc.WINDOWS, pc.DIGITS)
    assert {"VERIFY_BLOCK", "AGG_SCALAR_BLOCK", "AGG_MAX_PER_LANE"} <= set(k)


@pytest.mark.parametrize("name", NAMES)
def test_scalar_list_reaches_every_entry_a_canonical_scalar_can(name):
    r = pm.CURVES[name].r
    S = pc.scalar_list(name)
    assert all(0 <= s < r for s in S) and len(set(S)) == len(S)
    for must in (0, 1, 2, 15, 16, 17, r - 1, r - 2, (r - 1) // 2):
        assert must in S
    assert pc.top_nibble(r) == {"bls12_381": 7, "bn254": 3}[name]
    assert pc.selected_entries(S) == pc.reachable_entries(r)
    # what no scalar below r selects: the top window's digits above r's top nibble (the table dump alone sees them)
    assert ((pc.top_nibble(r) + 1) << 252) >= r
    assert len(pc.reachable_entries(r)) == 63 * 15 + pc.top_nibble(r)


@pytest.mark.parametrize("name", NAMES)
def test_model_table_and_generator_multiples(name):
    cp = pm.CURVES[name]
    G1 = pm.groups(cp)[0]
    tab = pc.model_table(cp, cp.g1)
    for w, d in [(0, 1), (0, 15), (1, 1), (5, 15), (63, 7), (63, 15)]:
        assert tab[w][d - 1] == G1.mul(cp.g1, d << (4 * w)), (w, d)
    assert all(p is None for row in pc.model_table(cp, None) for p in row)
    for s in (0, 1, cp.r - 1, 0xDEADBEEF << 200):
        assert pc.mul_g(name, s) == G1.mul(cp.g1, s)


@pytest.mark.parametrize("name", NAMES)
def test_rows_differ_lane_by_lane_and_mix_the_edges(name):
    r = pm.CURVES[name].r
    for key in (pc.key_random(name, 5), pc.key_equal_bases(name)):
        rows = pc.rows_for(key, 257)
        assert len(set(rows[:64])) == 64   # one wave: every lane its own row
        wave = {x for row in rows[:64] for x in row}
        assert {0, r - 1} <= wave
        for row, _ in key.collision_rows:
            assert tuple(row) in rows[:64]


@pytest.mark.parametrize("name", NAMES)
def test_crafted_keys_collide_where_they_say(name):
    r = pm.CURVES[name].r
    keys = pc.collision_keys(name)
    assert len(keys) == 8
    for key in keys:
        assert key.collision_rows, key
        for row, events in key.collision_rows:
            assert all(0 <= x < r for x in row)
            ch = key.chain(row)
            for j, w, kind in events:
                hit = [e for e in ch if e[0] == j and e[1] == w]
                assert len(hit) == 1 and hit[0][3] == kind, (key, j, w, kind, hit)
    # (d): equal inputs double at base 2's only entry, opposite inputs cancel at its last; ordinary bases follow both
    d = pc.key_equal_bases(name)
    assert d.g[0] == 0 and d.g[1] == d.g[2] and d.num_public == 5
    (same, _), (opp, _) = d.collision_rows
    assert same[0] == same[1] and (opp[0] + opp[1]) % r == 0
    assert [e[3] for e in d.chain(same)][:2] == ["take", "double"]
    assert any(e[0] > 1 for e in d.chain(same)) and any(e[0] > 1 for e in d.chain(opp))
    after = [e for e in d.chain(opp) if e[0] == 2]
    assert after[0][3] == "take"   # the accumulator was the identity after the cancellation
    # (e): the FIRST table addition is the collision, further additions follow
    for w, dgt in pc.collision_entries(name):
        for sign, kind in ((+1, "double"), (-1, "cancel")):
            k = pc.key_first_addition(name, w, dgt, sign)
            (row, _), = k.collision_rows
            ch = k.chain(row)
            assert ch[0] == (0, w, dgt, kind) and len(ch) > 8, (k, ch[:2])
            assert all(pc.nibble(row[0], v) == 0 for v in range(w)) and pc.nibble(row[0], w) == dgt
            if kind == "cancel":
                assert ch[1][3] == "take"
            assert k.g[0] == sign * (dgt << (4 * w)) * k.g[1] % r
    assert pc.collision_entries(name)[2] == (63, pc.top_nibble(r))
    # (f): IC is the identity, no term is, and the last addition is the cancellation
    f = pc.key_identity_ic(name)
    (row, _), = f.collision_rows
    assert f.num_public == 5 and f.ic_log(row) == 0 and f.expected_ic(row) is None
    assert f.g[0] and all(x * gj % r for x, gj in zip(row, f.g[1:]))
    assert f.chain(row)[-1][3] == "cancel" and [e[3] for e in f.chain(row)[:-1]].count("cancel") == 0


@pytest.mark.parametrize("name", NAMES)
def test_chain_agrees_with_the_group_law_on_points(name):
    """the replay on logarithms against the same replay on points (model table entries, affine additions) for one collision row"""
    cp = pm.CURVES[name]
    G1 = pm.groups(cp)[0]
    key = pc.key_first_addition(name, 5, 15, -1)
    (row, _), = key.collision_rows
    pts = key.points
    tabs = [pc.model_table(cp, p) for p in pts[1:]]
    acc = pts[0]
    for j, w, d, kind in key.chain(row):
        e = tabs[j][w][d - 1]
        assert {"take": acc is None, "double": acc == e, "cancel": acc == G1.neg(e), "add": acc is not None and acc[0] != e[0]}[kind]
        acc = G1.add(acc, e)
    assert acc == key.expected_ic(row)


@pytest.mark.parametrize("name", NAMES)
def test_identity_entries_of_keys_b_and_c(name):
    b, c = pc.key_identity_first(name), pc.key_identity_inside(name)
    assert b.points[0] is None and all(p is not None for p in b.points[1:])
    assert c.points[3] is None and sum(p is None for p in c.points) == 1
    assert not c.vk.gamma_abc_g1[3].any() and c.vk.gamma_abc_g1[2].any()
    assert [k.num_public for k in pc.all_keys(name)[:5]] == list(pc.NUM_PUBLIC)


@pytest.mark.parametrize("name", NAMES)
def test_exact_verdict_proofs_hold_in_the_exponent(name):
    """a b = alpha beta + gamma ic + c delta exactly at the honest row, and at no row with one x_j + 1"""
    r = pm.CURVES[name].r
    key = pc.key_random(name, 5)
    row = pc.rows_for(key, 3)[2]
    rng = pm.SplitMix64(0xAB0)
    a, b = rng.field(r - 1) + 1, 0xB0B
    c = (a * b - key.alpha * key.beta - key.gamma * key.ic_log(row)) * pow(key.delta, -1, r) % r
    from helpers import g1_to_arr
    L = key.cp.fq_limbs64
    proof = key.proof(row, 0)
    assert (proof[:2 * L] == g1_to_arr([pc.mul_g(name, a)], key.cp)[0]).all() and (proof[6 * L:] == g1_to_arr([pc.mul_g(name, c)], key.cp)[0]).all()
    assert (a * b - key.alpha * key.beta - key.gamma * key.ic_log(row) - c * key.delta) % r == 0
    for j in range(5):
        assert (a * b - key.alpha * key.beta - key.gamma * key.ic_log(pc.bump(row, j, r)) - c * key.delta) % r != 0


@pytest.mark.parametrize("name", NAMES)
def test_unreduced_rows_encode_x_plus_r(name):
    r = pm.CURVES[name].r
    arr, reduced = pc.unreduced_rows(name, [0, 1, r - 1, 0x1234567])
    assert arr.shape == (5, 1, 4) and reduced[:4] == [0, 1, r - 1, 0x1234567]
    for row, v in zip(arr, reduced):
        m = sum(int(row[0, k]) << (64 * k) for k in range(4))
        assert m >= r and m * pow(1 << 256, -1, r) % r == v
    assert (arr[4] == 2**64 - 1).all()
