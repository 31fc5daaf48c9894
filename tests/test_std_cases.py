"""CPU tier for tests/std_cases.py: the generators run (they assert every property a case is named after with the models alone, and on
every row of every product case that c1 + c2 < 2^32 and the running value < 2 p), the limb-level model of Fp::mul_cios32 is pinned
against plain a b R^-1 mod p and against the generated header's constants, the group model's scalar multiple against pymodel's, and
the operand file of tests/std_lab_replay.cpp is written from the host lab's outputs and checked for its layout."""
import os
import random
import re

import numpy as np
import pytest

import pymodel
import std_cases as sc

FIELDS = [(curve, which) for curve in sc.CURVES for which in ("fr", "fq")]


@pytest.mark.parametrize("curve,kind,form", sc.PARAMS, ids=["%s-%s-%s" % p for p in sc.PARAMS])
def test_generator(curve, kind, form):
    cases = sc.cases(curve, kind, form)
    fid, nin, nout = sc.slots(kind, form)
    assert len(cases) >= (256 if kind in ("fr", "fq", "fq2") else 24)
    assert all(len(c.slots) == nin for c in cases)


@pytest.mark.parametrize("curve,which", FIELDS)
def test_limb_model_is_the_montgomery_product(curve, which):
    """cios32 against a b R^-1 mod p: the value before the reduction is that or that + p, on named and seeded pairs; and the constants
    the model derives are the ones params_gen.hpp hands the C++"""
    f = sc.std(curve, which)
    p = f.p
    rng = random.Random("std/pin/%s" % f.name)
    prs = [(0, 0), (1, 1), (p - 1, p - 1), (f.Rp, f.Rp), (f.Rp, p - 1), (p - 1, 1)] + [(rng.randrange(p), rng.randrange(p)) for _ in range(200)]
    for a, b in prs:
        pre, rows = sc.cios32(f, a, b)
        assert len(rows) == f.N and pre < 2 * p and pre % p == a * b * pow(f.R, -1, p) % p
    assert sc.cios32(f, f.Rp, f.Rp)[0] % p == f.Rp and sc.cios32(f, 5, f.R * f.R % p)[0] % p == 5 * f.R % p
    hdr = open(os.path.join(sc.fc.ROOT, "groth16_amd", "csrc", "params_gen.hpp")).read()
    body = hdr[hdr.index("struct %sP" % (sc.fc.CURVE_KEY[curve] + ("Fq" if which == "fq" else "Fr"))):]
    body = body[:body.index("};")]
    assert re.search(r"\bN\s*=\s*%d\b" % f.N, body), "the word count of %s" % f.name
    assert re.search(r"INV\s*=\s*(0x%xu?|%du?)\b" % (f.INV, f.INV), body, re.I), "-p^-1 mod 2^32 of %s" % f.name


@pytest.mark.parametrize("curve,which", FIELDS)
def test_product_cases_hold_what_the_issue_names(curve, which):
    f = sc.std(curve, which)
    p = f.p
    prs = sc.product_pairs(curve, which)
    assert sum(1 for c in prs if p <= c[3] < 2 * p) >= 32 and sum(1 for c in prs if c[3] < p) >= 32
    assert any(c[0].startswith("searched: before the reduction in [p") for c in prs) and any(c[0].startswith("directed") and c[3] >= p for c in prs)
    zero_m = [c for c in prs if c[0].startswith("m = 0")]
    assert len(zero_m) == 4
    for what, a, b, pre in zero_m:
        assert any(r[0] == 0 for r in sc.cios32(f, a, b)[1]), what
    best = [c for c in prs if c[0].startswith("c1 + c2 reaches")]
    top = max(max(r[1] for r in sc.cios32(f, a, b)[1]) for _, a, b, _ in prs)
    assert len(best) == 16 and top == sc.MAX_C1C2[f.name] < 1 << 32
    # the bound the comment leans on: both carries stay below p's top word + 1, and twice that fits 32 bits for all four fields
    assert top <= 2 * (f.pw[-1] + 1) < 1 << 32
    print("%s: %d product pairs, largest c1 + c2 = 0x%x, 2 (top word of p + 1) = 0x%x" % (f.name, len(prs), top, 2 * (f.pw[-1] + 1)))
    names = {c[0] for c in sc.pairs(curve, which)}
    assert {"a + b = p", "a + b = p - 1", "a + b = p + 1", "a - b with a = b - 1"} <= names


@pytest.mark.parametrize("curve", sc.CURVES)
@pytest.mark.parametrize("g2", (0, 1))
def test_group_model_multiples(curve, g2):
    """the plain double-and-add of the affine model against pymodel's Group.mul on the generator (which reduces k mod r)"""
    g = sc.gctx(curve, g2)
    G = pymodel.groups(g.m.cp)[g2]
    rng = random.Random("std/mul/%s/%d" % (curve, g2))
    for k in (1, 2, 3, 255, g.r - 1, rng.randrange(g.r), rng.randrange(1 << 256)):
        assert g.mul(g.m.gen, k) == G.mul(g.m.gen, k % g.r), k
    assert g.mul(g.m.gen, g.r) is None and g.mul(None, 5) is None
    P = g.m.gen
    rec = g.raw(P, g.m.elem([rng.randrange(1, g.p) for _ in range(g.C)]))
    assert g.point_of(rec, "a scaled record") == P and g.point_of(g.raw(P, g.F.one), "scale 1") == P


def test_operand_dump_for_the_replay_program(tmp_path):
    """the file tests/std_lab_replay.cpp reads: one record per (curve, kind, form), operands and this build's outputs"""
    path = tmp_path / "std_lab.bin"
    records, tuples = sc.dump_operands(str(path), sc.run_host)
    assert records == len(sc.PARAMS) == 2 * (2 * 13 + 7 + 2 * 7)
    words = np.fromfile(str(path), dtype="<u4")
    pos = total = 0
    for curve, kind, form in sc.PARAMS:
        cid, k, fid, cnt, nin, nout, N = (int(x) for x in words[pos:pos + 7])
        assert (cid, k, fid, nin, nout, N) == (sc.fc.CURVE_ID[curve], sc.KIND[kind], *sc.slots(kind, form), sc.words_per_slot(curve, kind))
        assert cnt == len(sc.cases(curve, kind, form))
        pos += 7 + cnt * (nin + nout) * N
        total += cnt
    assert pos == len(words) and total == tuples
    print("std_lab.bin: %d records, %d tuples" % (records, tuples))


@pytest.mark.parametrize("curve", sc.CURVES)
def test_fixed_base_generators(curve):
    """tests/fixed_base_cases.py (the GPU tier's test_gpu_fixed_base.py): the generators assert which table entries a scalar reads"""
    import fixed_base_cases as fb

    ks = fb.single_scalars(curve)
    assert len(ks) == 45 and {fb.table_entries(k)[0] // fb.DIGITS for n, k in ks if n.startswith("one non-zero byte")} == set(range(32))
    assert len(fb.window_cases(curve)) == 15 and len(fb.size_cases(curve)) == 12
    for nw in (None, 0, 1):
        cs, want = fb.qap_circuit(curve, 0x1234567890ABCDEF, nw)
        assert len(want) == (4 if nw is None else nw) and cs.num_witness == (5 if nw is None else nw)
