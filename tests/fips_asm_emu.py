"""An emulator of the generated field assembly (TEST INFRASTRUCTURE): groth16_amd/csrc/fips_asm_gen.hpp parsed as text -- the asm
strings, the output / input / clobber lists and the literal constants -- and executed with u32 / u64 register semantics.  The
generator is never run: what is checked is the header the kernels are compiled from.

Three passes over a block:
  * check_static   straight-line data flow: no read of a register before it is written, no physical register outside the clobber
                   list, no write to an input, and an output may only be written while inputs are still to be read if it is declared
                   early-clobber ("=&v");
  * run            concrete values.  Every v_mad_u64_u32 must leave no carry (the block sends it to vcc and nobody reads it), no
                   v_sub_u32 may borrow, no add / shift form may wrap 32 bits;
  * bounds         the plan's own assumptions (fp30.hpp, fips_plan): every operand limb and every m_i anywhere in [0, 2^30 - 1], the
                   real p and K p limbs.  Intervals are propagated through the same instructions; every accumulator must stay below
                   2^64.  32-bit results that this all-ones worst case cannot bound are returned as `value_bounded`: they hold only
                   because the VALUE is bounded, and the concrete extremes have to vouch for them.
An unknown opcode is an error in every pass.
"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "groth16_amd", "csrc", "fips_asm_gen.hpp")
W32 = (1 << 32) - 1
LIM64 = 1 << 64

OPCODES = ("v_mad_u64_u32", "v_mul_lo_u32", "v_and_b32", "v_lshrrev_b64", "v_alignbit_b32", "v_sub_u32", "v_lshl_add_u32",
           "v_add_u32", "v_lshlrev_b32", "s_mov_b32")


class EmuError(AssertionError):
    pass


class Block:
    def __init__(self, struct, name):
        self.struct, self.name = struct, name
        self.text = []        # instruction strings
        self.outs = []        # (constraint, expression)
        self.ins = []
        self.clobbers = []
        self.instrs = []      # decoded: (opcode, [operands]); operand = ("o", n) | ("v", n) | ("vp", n) | ("s", n) | ("vcc",) | ("i", value)
        self.column = []      # column of the product each instruction works on (2 NL - 1: the top limb's own tail)
        self._fn = None

    @property
    def label(self):
        return "%s::%s" % (self.struct, self.name)

    def where(self, i):
        return "%s instruction %d (column %d) `%s`" % (self.label, i, self.column[i], self.text[i])


def _operand(tok, blk):
    tok = tok.strip()
    m = re.fullmatch(r"%(\d+)", tok)
    if m:
        return ("o", int(m.group(1)))
    m = re.fullmatch(r"v\[(\d+):(\d+)\]", tok)
    if m:
        if int(m.group(2)) != int(m.group(1)) + 1:
            raise EmuError("%s: odd register pair %s" % (blk.label, tok))
        return ("vp", int(m.group(1)))
    m = re.fullmatch(r"v(\d+)", tok)
    if m:
        return ("v", int(m.group(1)))
    m = re.fullmatch(r"s(\d+)", tok)
    if m:
        return ("s", int(m.group(1)))
    if tok == "vcc":
        return ("vcc",)
    if re.fullmatch(r"0x[0-9a-fA-F]+|\d+", tok):
        return ("i", int(tok, 0))
    raise EmuError("%s: cannot parse operand %r" % (blk.label, tok))


def _split_list(s):
    return [x.strip() for x in re.findall(r'"[^"]*"(?:\([^)]*\))?', s)]


def parse_header(path=HEADER):
    """every inline-assembly block of the header, in order"""
    blocks, struct, blk, stage = [], None, None, 0
    for line in open(path).read().splitlines():
        s = line.strip()
        m = re.match(r"template <> struct FipsAsm<(\w+)>", s)
        if m:
            struct = m.group(1)
            continue
        m = re.match(r"static __device__ __forceinline__ void (\w+)\(", s)
        if m:
            blk, stage = Block(struct, m.group(1)), 0
            continue
        if blk is None:
            continue
        if s == "asm(":
            stage = 1
        elif stage == 1 and s.startswith('"'):
            m = re.fullmatch(r'"(.*)\\n"', s)
            if not m:
                raise EmuError("%s: unexpected asm line %r" % (blk.label, s))
            blk.text.append(m.group(1))
        elif stage >= 1 and s.startswith(":"):
            items = _split_list(s[1:-2] if s.endswith(");") else s[1:])
            if stage == 1:
                blk.outs = [re.fullmatch(r'"([^"]*)"\((.*)\)', x).groups() for x in items]
            elif stage == 2:
                blk.ins = [re.fullmatch(r'"([^"]*)"\((.*)\)', x).groups() for x in items]
            else:
                blk.clobbers = [x.strip('"') for x in items]
                _decode(blk)
                blocks.append(blk)
                blk = None
            stage += 1
    return blocks


def _decode(blk):
    col = 0
    for t in blk.text:
        op, _, rest = t.partition(" ")
        if op not in OPCODES:
            raise EmuError("%s: unknown opcode in `%s`" % (blk.label, t))
        blk.instrs.append((op, [_operand(x, blk) for x in rest.split(",")]))
        blk.column.append(col)
        if op in ("v_lshrrev_b64", "v_alignbit_b32"):   # the shift that ends a column; what follows seeds the next one
            col += 1


def _halves(o):
    """the 32-bit registers an operand names"""
    if o[0] == "vp":
        return [("v", o[1]), ("v", o[1] + 1)]
    return [o] if o[0] in ("v", "s", "o") else []


def _dst_src(op, ops):
    """(destination operands, source operands) of a decoded instruction"""
    if op == "v_mad_u64_u32":
        return [ops[0], ops[1]], ops[2:]
    return [ops[0]], ops[1:]


def check_static(blk):
    n_out = len(blk.outs)
    n_ops = n_out + len(blk.ins)
    clob = set(blk.clobbers)
    written = set()
    last_input_read = -1
    first_write = {}
    for i, (op, ops) in enumerate(blk.instrs):
        dst, src = _dst_src(op, ops)
        for o in src:
            for r in _halves(o):
                if r[0] == "o":
                    if r[1] >= n_ops:
                        raise EmuError("%s: operand %%%d does not exist" % (blk.where(i), r[1]))
                    if r[1] < n_out and r not in written:
                        raise EmuError("%s: output %%%d is read before it is written" % (blk.where(i), r[1]))
                    if r[1] >= n_out:
                        last_input_read = i
                elif r not in written:
                    raise EmuError("%s: %s%d is read before it is written" % (blk.where(i), r[0], r[1]))
        for o in dst:
            if o[0] == "vcc":
                if "vcc" not in clob:
                    raise EmuError("%s: vcc is written but not clobbered" % blk.where(i))
                continue
            if o[0] == "i":
                raise EmuError("%s: an immediate as destination" % blk.where(i))
            for r in _halves(o):
                if r[0] == "o":
                    if r[1] >= n_out:
                        raise EmuError("%s: input %%%d is written" % (blk.where(i), r[1]))
                    first_write.setdefault(r[1], i)
                elif "%s%d" % r not in clob:
                    raise EmuError("%s: physical register %s%d is outside the clobber list" % (blk.where(i), r[0], r[1]))
                written.add(r)
    for k, (cons, expr) in enumerate(blk.outs):
        if not cons.startswith("="):
            raise EmuError("%s: output %d has constraint %r" % (blk.label, k, cons))
        if "&" not in cons and k in first_write and first_write[k] < last_input_read:
            raise EmuError("%s: output %%%d (%s) is written at instruction %d while inputs are still read (up to %d) but is not "
                           "early-clobber" % (blk.label, k, expr, first_write[k], last_input_read))
    for cons, expr in blk.ins:
        if cons not in ("v", "s"):
            raise EmuError("%s: input constraint %r" % (blk.label, cons))


# ---- concrete mode: the block compiled to one straight-line Python function -------------------------------------------------------
def _name(r):
    return "%s%d" % r


def _rd(o):
    if o[0] == "i":
        return str(o[1])
    if o[0] == "vp":
        return "p%d" % o[1]
    if o[0] == "v":      # a half of an accumulator pair, or a register of its own
        return None
    return _name(o)


def _compile(blk):
    pairs = set()
    for op, ops in blk.instrs:
        for o in ops:
            if o[0] == "vp":
                pairs.add(o[1])

    def rd(o):
        if o[0] == "v":
            if o[1] in pairs:
                return "(p%d & 0xffffffff)" % o[1]
            if o[1] - 1 in pairs:
                return "(p%d >> 32)" % (o[1] - 1)
            return "v%d" % o[1]
        return _rd(o)

    def wr(o, i):
        if o[0] == "v" and (o[1] in pairs or o[1] - 1 in pairs):
            raise EmuError("%s: a half of an accumulator pair is written on its own" % blk.where(i))
        return "p%d" % o[1] if o[0] == "vp" else _name(o)

    n_out = len(blk.outs)
    src = ["def run(I, fail, seen):"]
    for k in range(len(blk.ins)):
        src.append("    o%d = I[%d]" % (n_out + k, k))
    for k in range(n_out):
        src.append("    o%d = None" % k)
    for i, (op, ops) in enumerate(blk.instrs):
        if op == "v_mad_u64_u32":
            src.append("    t = %s * %s + %s" % (rd(ops[2]), rd(ops[3]), rd(ops[4])))
            src.append("    if t >> 64: fail(%d, 'carry out of v_mad_u64_u32', t)" % i)
            src.append("    %s = t" % wr(ops[0], i))
        elif op == "v_mul_lo_u32":
            src.append("    %s = (%s * %s) & 0xffffffff" % (wr(ops[0], i), rd(ops[1]), rd(ops[2])))
        elif op == "v_and_b32":
            src.append("    %s = %s & %s" % (wr(ops[0], i), rd(ops[1]), rd(ops[2])))
        elif op == "v_lshrrev_b64":
            src.append("    %s = %s >> %s" % (wr(ops[0], i), rd(ops[2]), rd(ops[1])))
        elif op == "v_alignbit_b32":
            src.append("    t = ((%s << 32) | %s) >> %s" % (rd(ops[1]), rd(ops[2]), rd(ops[3])))
            src.append("    if t >> 32: fail(%d, 'the shifted accumulator does not fit 32 bits (v_alignbit_b32 drops the rest)', t)" % i)
            src.append("    if t > seen.get(%d, -1): seen[%d] = t" % (i, i))
            src.append("    %s = t" % wr(ops[0], i))
        elif op == "v_sub_u32":
            src.append("    t = %s - %s" % (rd(ops[1]), rd(ops[2])))
            src.append("    if t < 0: fail(%d, 'borrow in v_sub_u32', t)" % i)
            src.append("    if t < seen.get(('min', %d), 1 << 32): seen[('min', %d)] = t" % (i, i))
            src.append("    %s = t" % wr(ops[0], i))
        elif op in ("v_lshl_add_u32", "v_add_u32", "v_lshlrev_b32"):
            if op == "v_lshl_add_u32":
                src.append("    t = (%s << %s) + %s" % (rd(ops[1]), rd(ops[2]), rd(ops[3])))
            elif op == "v_add_u32":
                src.append("    t = %s + %s" % (rd(ops[1]), rd(ops[2])))
                src.append("    if t > seen.get(%d, -1): seen[%d] = t" % (i, i))
            else:
                src.append("    t = %s << %s" % (rd(ops[2]), rd(ops[1])))
            src.append("    if t >> 32: fail(%d, '32-bit wrap in %s', t)" % (i, op))
            src.append("    %s = t" % wr(ops[0], i))
        elif op == "s_mov_b32":
            src.append("    %s = %s" % (wr(ops[0], i), rd(ops[1])))
        else:
            raise EmuError("%s: unknown opcode" % blk.where(i))
    src.append("    return (%s,)" % ", ".join("o%d" % k for k in range(n_out)))
    ns = {}
    exec(compile("\n".join(src), "<%s>" % blk.label, "exec"), ns)
    return ns["run"]


def input_values(blk, arrays):
    """the block's input list for named operand arrays ({"x0": limbs, ...}); literal constants come from the header itself"""
    vals = []
    for cons, expr in blk.ins:
        m = re.fullmatch(r"(\w+)\[(\d+)\]", expr)
        if m:
            vals.append(int(arrays[m.group(1)][int(m.group(2))]))
        else:
            m = re.fullmatch(r"(0x[0-9a-fA-F]+|\d+)u?", expr)
            if not m:
                raise EmuError("%s: cannot read input %r" % (blk.label, expr))
            vals.append(int(m.group(1), 0))
    return vals


def run(blk, arrays, seen=None):
    """execute the block on concrete operand limbs; returns {"r": [...], ("t": [...])} -- the output arrays.  `seen` collects, per
    instruction index i, the largest result of the shifts and adds that write a top limb (seen[i]) and the smallest difference of
    every v_sub_u32 (seen[("min", i)])"""
    if blk._fn is None:
        blk._fn = _compile(blk)

    def fail(i, what, t):
        raise EmuError("%s: %s (value 0x%x); operands %s" % (blk.where(i), what, t, {k: [hex(int(x)) for x in v] for k, v in arrays.items()}))
    for k, v in arrays.items():
        if any(not 0 <= int(x) <= W32 for x in v):
            raise EmuError("%s: operand %s is not a list of 32-bit limbs" % (blk.label, k))
    res = blk._fn(input_values(blk, arrays), fail, seen if seen is not None else {})
    out = {}
    for (cons, expr), v in zip(blk.outs, res):
        name, idx = re.fullmatch(r"(\w+)\[(\d+)\]", expr).groups()
        out.setdefault(name, {})[int(idx)] = v
    return {k: [d.get(i) for i in range(max(d) + 1)] for k, d in out.items()}


# ---- bound mode -----------------------------------------------------------------------------------------------------------------
def bounds(blk, limb_max=(1 << 30) - 1):
    """interval propagation under the plan's assumptions.  Returns (margin_bits, worst, value_bounded): the tightest accumulator
    margin as log2(2^64 / largest accumulator bound), the instruction index that has it, and the list of (index, reason) of 32-bit
    results the all-ones worst case cannot bound.  Raises EmuError if an accumulator can reach 2^64."""
    import math
    n_out = len(blk.outs)
    reg = {}
    for k, (cons, expr) in enumerate(blk.ins):
        m = re.fullmatch(r"(0x[0-9a-fA-F]+|\d+)u?", expr)
        reg[("o", n_out + k)] = (int(m.group(1), 0),) * 2 if m else (0, limb_max)
    worst, worst_i, vb = 0, -1, []

    def rd(o):
        if o[0] == "i":
            return (o[1], o[1])
        if o[0] == "vp":
            return reg[o]
        if o[0] == "v":
            if ("vp", o[1]) in reg:
                lo, hi = reg[("vp", o[1])]
                return (lo, hi) if hi <= W32 else (0, W32)
            if ("vp", o[1] - 1) in reg:
                lo, hi = reg[("vp", o[1] - 1)]
                return (lo >> 32, hi >> 32)
        return reg[o]

    for i, (op, ops) in enumerate(blk.instrs):
        if op == "v_mad_u64_u32":
            a, b, c = rd(ops[2]), rd(ops[3]), rd(ops[4])
            t = (a[0] * b[0] + c[0], a[1] * b[1] + c[1])
            if t[1] >= LIM64:
                raise EmuError("%s: the accumulator's bound 2^%.3f reaches 2^64 under the plan's assumptions" % (blk.where(i), math.log2(t[1])))
            if t[1] > worst:
                worst, worst_i = t[1], i
            reg[ops[0]] = t
        elif op == "v_mul_lo_u32":
            reg[ops[0]] = (0, W32)
        elif op == "v_and_b32":
            a, b = rd(ops[1]), rd(ops[2])
            reg[ops[0]] = (0, min(a[1], b[1]))
        elif op == "v_lshrrev_b64":
            s, a = rd(ops[1])[0], rd(ops[2])
            reg[ops[0]] = (a[0] >> s, a[1] >> s)
        elif op == "v_alignbit_b32":
            hi, lo, s = rd(ops[1]), rd(ops[2]), rd(ops[3])[0]
            full = reg[("vp", ops[2][1])] if ops[2][0] == "v" and ("vp", ops[2][1]) in reg else None
            t = (full[0] >> s, full[1] >> s) if full else (0, ((hi[1] << 32) | lo[1]) >> s)
            if t[1] > W32:
                vb.append((i, "the last carry is the top limb: it fits 32 bits because the value is bounded, not in this worst case"))
                t = (0, W32)
            reg[ops[0]] = t
        elif op == "v_sub_u32":
            a, b = rd(ops[1]), rd(ops[2])
            if a[0] < b[1]:
                vb.append((i, "K p's top limb minus the subtrahend's: no borrow because the subtrahend's VALUE is below K p"))
            reg[ops[0]] = (max(a[0] - b[1], 0), a[1] - b[0])
        elif op in ("v_lshl_add_u32", "v_add_u32", "v_lshlrev_b32"):
            if op == "v_lshl_add_u32":
                a, s, b = rd(ops[1]), rd(ops[2])[0], rd(ops[3])
                t = ((a[0] << s) + b[0], (a[1] << s) + b[1])
            elif op == "v_add_u32":
                a, b = rd(ops[1]), rd(ops[2])
                t = (a[0] + b[0], a[1] + b[1])
            else:
                s, a = rd(ops[1])[0], rd(ops[2])
                t = (a[0] << s, a[1] << s)
            if t[1] > W32:
                vb.append((i, "the top limb plus its difference: no wrap because the value is bounded"))
                t = (0, W32)
            reg[ops[0]] = t
        elif op == "s_mov_b32":
            reg[ops[0]] = rd(ops[1])
        else:
            raise EmuError("%s: unknown opcode" % blk.where(i))
    return math.log2(LIM64 / worst), worst_i, vb
