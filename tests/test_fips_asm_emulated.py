"""CPU tier: the 32 inline-assembly blocks of fips_asm_gen.hpp, executed instruction by instruction (tests/fips_asm_emu.py) on the
shared edge cases (tests/fp30_cases.py) against the big-int model, and the host field lab (g16_host_fp30_op) against both.

Every kernel's field arithmetic goes through these blocks, they are compiled for the device only, and they are built to the edge: a
v_mad_u64_u32's carry goes to vcc and nobody reads it, the fused subtractions are unchecked 32-bit differences, and the top limb fits
32 bits only because the value is bounded.  A failure here names the block, the instruction, its column and the operands.

value_bounded() lists the instructions whose 32-bit result the plan's own worst case (every limb 2^30 - 1) cannot bound; bound mode
must find exactly those, and the concrete extremes run them with the wrap / borrow assertions live."""
import ctypes as C
import os

import numpy as np
import pytest

import fips_asm_emu as emu
import fp30_cases as fc

FIELDS = {f.struct: f for f in fc.fields()}
BLOCKS = emu.parse_header()
BLOCK_IDS = [b.label for b in BLOCKS]
MARGINS = {}   # block label -> (bits of head room of the tightest accumulator in bound mode, instruction index)


def margin_text(blk):
    if blk.label not in MARGINS:
        try:
            MARGINS[blk.label] = emu.bounds(blk)[:2]
        except emu.EmuError as e:
            return "bound mode fails: %s" % e
    bits, i = MARGINS[blk.label]
    return "tightest accumulator margin in bound mode: %.6f bits below 2^64 at %s" % (bits, blk.where(i))


def value_bounded(blk):
    """(opcode, column, reason) of the instructions that bound mode cannot vouch for: they hold only because the VALUE is bounded.
    In the four-sweep blocks the shift that takes the top limb out of the last column's accumulator (fp30.hpp, the comment that
    closes fips_plan: the all-ones worst case sums to several R'; with one or two sweeps even that worst case fits 32 bits).  In
    the blocks with a fused subtraction the top limb's difference: K p's top limb minus the subtrahend's does not borrow because
    the subtrahend is below K p as a VALUE -- a normalised top limb alone could be anything."""
    nl = FIELDS[blk.struct].NL
    if blk.name == "mul4":
        return [("v_alignbit_b32", 2 * nl - 2, "the last carry is the top limb: < 2^32 because callers keep sum A B p / R' <= 0.5")]
    if blk.name.endswith(("_s2", "_s4", "_s8", "_x3")):
        return [("v_sub_u32", 2 * nl - 1, "top(K p) - 1 >= the subtrahend's top limb: s < 1.5 p < K p (u + 2 v < 4.5 p < 6 p for x3)")]
    return []


def arrays_for(blk, ops, f):
    """operand tuple (x0 [y0] [x1 y1 ...] [s0 [s1]]) -> the block's named arrays"""
    ns, sqr, sub, _ = fc.PRODUCT_FORMS[blk.name]
    names = []
    for k in range(ns):
        names.append("x%d" % k)
        if not sqr:
            names.append("y%d" % k)
    names += ["s0"] if sub == "k" else ["s0", "s1"] if sub == "x3" else []
    assert len(names) == len(ops)
    return {n: f.limbs(v) for n, v in zip(names, ops)}


def test_header_has_the_32_blocks():
    per = {}
    for b in BLOCKS:
        per.setdefault(b.struct, []).append(b.name)
    assert len(BLOCKS) == 32
    assert set(per) == set(FIELDS)
    for struct, names in per.items():
        assert sorted(names) == sorted(fc.product_forms(FIELDS[struct])), struct
        assert len(names) == (12 if struct.endswith("FqP") else 4)
    used = {op for b in BLOCKS for op, _ in b.instrs}
    assert used <= set(emu.OPCODES) and len(emu.OPCODES) == 10


@pytest.mark.parametrize("blk", BLOCKS, ids=BLOCK_IDS)
def test_static_data_flow(blk):
    emu.check_static(blk)
    f = FIELDS[blk.struct]
    assert [e for _, e in blk.outs][:f.NL] == ["r[%d]" % i for i in range(f.NL)]


@pytest.mark.parametrize("blk", BLOCKS, ids=BLOCK_IDS)
def test_bound_mode_keeps_every_accumulator_below_2_64(blk):
    bits, worst, vb = emu.bounds(blk)
    MARGINS[blk.label] = (bits, worst)
    print("%-28s %s" % (blk.label, margin_text(blk)))
    assert bits > 0, margin_text(blk)
    found = sorted((blk.instrs[i][0], blk.column[i]) for i, _ in vb)
    assert found == sorted((op, col) for op, col, _ in value_bounded(blk)), (blk.label, [(blk.where(i), why) for i, why in vb])


@pytest.mark.parametrize("blk", BLOCKS, ids=BLOCK_IDS)
def test_emulated_block_equals_the_model(blk):
    f = FIELDS[blk.struct]
    cases = fc.product_cases(f, blk.name)
    assert len(cases) >= 256
    seen = {}
    try:
        for ops, want in cases:
            got = emu.run(blk, arrays_for(blk, ops, f), seen)["r"]
            assert got == f.limbs(want), "%s%s: got %s, model %s" % (blk.label, tuple(hex(x) for x in ops), got, f.limbs(want))
    except AssertionError as e:
        raise AssertionError("%s\n%s" % (e, margin_text(blk))) from None
    # the instruction that writes the top limb saw the lazy range: the largest top limb of the model, at least p's own
    last = len(blk.instrs) - 1
    assert blk.instrs[last][0] in ("v_alignbit_b32", "v_add_u32") and blk.instrs[last][1][0] == ("o", f.NL - 1), blk.where(last)
    assert seen[last] == max(f.limbs(w)[-1] for _, w in cases) >= f.p >> f.top_shift, (blk.label, hex(seen[last]), margin_text(blk))
    # ... and the concrete extremes reached the EDGE of every value-bounded instruction
    for op, col, _ in value_bounded(blk):
        (i,) = [k for k in range(len(blk.instrs)) if (blk.instrs[k][0], blk.column[k]) == (op, col)]
        if op == "v_alignbit_b32":
            assert i == last   # its largest result is the model's largest top limb: asserted above
        else:
            # the top limb's difference came down to  top(K p constant) - the largest top limb the precondition admits:
            # s < 1.5 p gives s_top <= (ceil(1.5 p) - 1) >> 30 (NL - 1); the x3 forms subtract u + 2 v, three times that
            kp_top = emu.input_values(blk, {n: [0] * f.NL for n in arrays_for(blk, cases[0][0], f)})[-1]
            s_top = (f.bound(fc.Fraction(3, 2)) - 1) >> f.top_shift
            assert seen[("min", i)] == kp_top - (3 if blk.name.endswith("_x3") else 1) * s_top >= 0, (blk.where(i), seen[("min", i)], kp_top, s_top)


# ---- the host lab against the model and, where a form has a block, against the emulated assembly -----------------------------------
def host_lab(lib, f, form, cases):
    fid, nin, nout = fc.LAB[form]
    ops = np.ascontiguousarray(np.array([[s for s in c.slots] for c in cases], dtype=np.uint32))
    assert ops.shape == (len(cases), nin, f.NL), (form, ops.shape)
    out = np.full((len(cases), nout, f.NL), 0xDEADBEEF, dtype=np.uint32)
    u32p = C.POINTER(C.c_uint32)
    rc = lib.c.g16_host_fp30_op(fc.CURVE_ID[f.curve], fc.FIELD_ID[f.which], fid, ops.ctypes.data_as(u32p), len(cases), out.ctypes.data_as(u32p))
    assert rc == 0, (f.name, form, rc)
    return out


@pytest.fixture(scope="module")
def lib():
    import groth16_amd

    return groth16_amd.lib()


@pytest.mark.parametrize("f", fc.fields(), ids=lambda f: f.name)
def test_host_lab_equals_the_model(lib, f):
    for form in fc.lab_forms(f, host=True):
        cases = fc.lab_cases(f, form)
        out = host_lab(lib, f, form, cases)
        for c, o in zip(cases, out):
            c.check(o)


@pytest.mark.parametrize("blk", BLOCKS, ids=BLOCK_IDS)
def test_host_lab_equals_the_emulated_assembly(lib, blk):
    f = FIELDS[blk.struct]
    cases = fc.product_cases(f, blk.name)
    lab = [fc.LabCase([f.limbs(x) for x in ops], None, blk.name) for ops, _ in cases]
    out = host_lab(lib, f, blk.name, lab)
    for (ops, want), o in zip(cases, out):
        got = emu.run(blk, arrays_for(blk, ops, f))["r"]
        assert [int(x) for x in o[0]] == got == f.limbs(want), (blk.label, [hex(x) for x in ops])


def test_host_lab_rejects_what_it_does_not_have(lib):
    u32p = C.POINTER(C.c_uint32)
    buf = np.zeros(16 * 13, dtype=np.uint32)
    p = buf.ctypes.data_as(u32p)
    assert lib.c.g16_host_fp30_op(0, 0, 4, p, 1, p) != 0       # the fused subtractions are base-field forms
    assert lib.c.g16_host_fp30_op(0, 1, 27, p, 1, p) != 0      # sub_pow2 is a scalar-field form
    assert lib.c.g16_host_fp30_op(0, 1, 72, np.zeros(21 * 13, dtype=np.uint32).ctypes.data_as(u32p), 1, p) != 0   # the lane pair's accumulator needs lanes
    assert lib.c.g16_host_fp30_op(0, 1, 12, p, 1, p) != 0 and lib.c.g16_host_fp30_op(0, 2, 0, p, 1, p) != 0
    assert lib.c.g16_host_fp30_op(7, 1, 0, p, 1, p) != 0 and lib.c.g16_host_fp30_op(0, 1, 0, p, 0, p) != 0
    assert os.path.exists(emu.HEADER)
