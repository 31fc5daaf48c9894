"""CPU tier for tests/table_cases.py: the generators run (they assert every property a case is named after with the model alone), the
affine model is pinned against pymodel's independent Jacobian group law, the operand lists hold what they must, the table lab's
layouts put every point class on both edges of a wave, and the operand file of tests/field_lab_replay.cpp is written from the host
lab's outputs and checked for its layout.  The host twins themselves are compared with the model by
test_fips_asm_emulated.py::test_host_lab_equals_the_model, which picks the new forms up from fp30_cases.LAB."""
import ctypes as C

import numpy as np
import pytest

import fp30_cases as fc
import pymodel
import table_cases as tc

FQ = [f for f in fc.fields() if f.which == "fq"]
PARAMS = [(f, form) for f in FQ for form in fc.TABLE_FORMS]
CONFIGS = [(curve, g2) for curve in fc.CURVE_ID for g2 in (0, 1)]


@pytest.mark.parametrize("f,form", PARAMS, ids=["%s-%s" % (f.name, form) for f, form in PARAMS])
def test_generator(f, form):
    cases = fc.lab_cases(f, form)
    fid, nin, nout = fc.LAB[form]
    assert len(cases) >= 65 and form in fc.lab_forms(f) and (form in fc.lab_forms(f, host=True)) == (form not in fc.DEVICE_ONLY)
    assert all(len(c.slots) == nin for c in cases)
    assert not any(form in fc.lab_forms(g) for g in fc.fields() if g.which == "fr")


@pytest.mark.parametrize("f", FQ, ids=lambda f: f.name)
def test_inverse_operands(f):
    p, B = f.p, 1 << (30 * f.NL - 3)
    ops = tc.inverse_operands(f)
    have = set(ops)
    assert len(have) == len(ops) and all(0 <= x < B for x in ops)
    assert {0, 1, 2, 3, p - 1, p - 2, (p + 1) // 2, (p - 1) // 2, f.R % p, B - 1, B - 2} <= have
    kmax = (B - 1) // p
    assert kmax >= 2 and all(k * p + d in have for k in range(1, kmax) for d in (-1, 0, 1)) and kmax * p in have
    assert all((1 << k) in have and (1 << k) - 1 in have for k in range(30 * f.NL - 3))
    assert all((fc.MASK << (30 * i)) in have for i in range(f.NL - 1))
    assert sum(1 for x in ops if x % p == 0) == kmax + 1


@pytest.mark.parametrize("curve,g2", CONFIGS)
def test_model_is_pymodels_group_law(curve, g2):
    """the affine chord / tangent rule against pymodel's Jacobian formulas on curve points (a modulus no scalar reaches, as in
    tests/subgroup_cases.model_groups: nothing is reduced modulo r)"""
    m = tc.model(curve, g2)
    cp = m.cp
    G = pymodel.Group(m.F, cp.b2 if g2 else cp.b1, 1 << 4096)
    mult = dict(tc.point_classes(curve, g2))["multiple of the generator"]
    for i, P in enumerate(mult):
        assert P == G.mul(m.gen, i + 1)
        for k in (1, 5, 20, 248):
            assert m.chain(P, k) == G.mul(P, 1 << k)
    assert m.add(mult[2], mult[6]) == G.add(mult[2], mult[6]) and m.add(mult[2], m.neg(mult[2])) is None and m.add(None, mult[1]) == mult[1]


@pytest.mark.parametrize("curve,g2", CONFIGS)
def test_table_layouts(curve, g2):
    big, T = tc.big_n(g2), tc.tasks_per_wave(g2)
    lanes = big * (2 if g2 else 1)
    assert 2 * tc.TABLE_THREADS < lanes <= 3 * tc.TABLE_THREADS and lanes % tc.TABLE_THREADS
    names = [name for name, _ in tc.point_classes(curve, g2)]
    assert len(names) == (9 if g2 else 4)
    first, last = set(), set()
    for layout in range(tc.layouts(curve, g2)):
        pts, edges = tc.table_points(curve, g2, big, layout)
        assert len(pts) == big
        cls = {P: name for name, cl in tc.point_classes(curve, g2) for P in cl}
        for t, name in edges.items():
            assert cls[pts[t]] == name and t % T in (0, T - 1)
            (first if t % T == 0 else last).add(name)
    assert first == last == set(names)
    for n in tc.SIZES:
        assert len(tc.table_points(curve, g2, n)[0]) == n
    m = tc.model(curve, g2)
    rows = tc.expected_table(curve, g2, tc.pool(curve, g2), 5, 3)
    two = dict(tc.point_classes(curve, g2))["(x, 0)"][0]
    i = tc.pool(curve, g2).index(two)
    assert any(rows[0][i]) and not any(rows[1][i]) and not any(rows[2][i])       # row 0 finite, every later row the identity
    assert tc.decode_row(m, rows[0][i]) == two and tc.decode_row(m, rows[1][i]) is None
    assert tc.abi_words(m, None) == [0] * len(tc.abi_words(m, two))


def run_host(f, form, cases):
    import groth16_amd

    lib = groth16_amd.lib()
    fid, nin, nout = fc.LAB[form]
    ops = np.ascontiguousarray(np.array([c.slots for c in cases], dtype=np.uint32))
    out = np.full((len(cases), nout, f.NL), 0xDEADBEEF, dtype=np.uint32)
    u32p = C.POINTER(C.c_uint32)
    rc = lib.c.g16_host_fp30_op(fc.CURVE_ID[f.curve], fc.FIELD_ID[f.which], fid, ops.ctypes.data_as(u32p), len(cases), out.ctypes.data_as(u32p))
    assert rc == 0, (f.name, form, rc)
    return out


def test_operand_dump_for_the_replay_program(tmp_path):
    """the file tests/field_lab_replay.cpp reads: one record per (base field, host form), operands and this build's outputs"""
    path = tmp_path / "field_lab.bin"
    records, tuples = tc.dump_operands(str(path), run_host)
    host_forms = [form for form in fc.TABLE_FORMS if form not in fc.DEVICE_ONLY]
    assert records == len(FQ) * len(host_forms) == 10
    words = np.fromfile(str(path), dtype="<u4")
    pos = total = 0
    for f in FQ:
        for form in host_forms:
            cid, field, fid, cnt, nin, nout, NL = (int(x) for x in words[pos:pos + 7])
            assert (cid, field, fid, nin, nout, NL) == (fc.CURVE_ID[f.curve], 1, *fc.LAB[form], f.NL) and cnt == len(fc.lab_cases(f, form))
            pos += 7 + cnt * (nin + nout) * NL
            total += cnt
    assert pos == len(words) and total == tuples
    print("field_lab.bin: %d records, %d tuples" % (records, tuples))


def test_the_device_only_forms_have_no_host_twin():
    import groth16_amd

    lib = groth16_amd.lib()
    u32p = C.POINTER(C.c_uint32)
    buf = np.zeros(16 * 13, dtype=np.uint32)
    p = buf.ctypes.data_as(u32p)
    for form in fc.DEVICE_ONLY:
        assert lib.c.g16_host_fp30_op(0, 1, fc.LAB[form][0], p, 1, p) != 0, form
    for fid in (80, 81, 82, 83, 85):
        assert lib.c.g16_host_fp30_op(0, 0, fid, p, 1, p) != 0, fid      # base-field forms
    assert lib.c.g16_host_fp30_op(0, 1, 87, p, 1, p) != 0 and lib.c.g16_host_fp30_op(0, 1, 79, p, 1, p) != 0
