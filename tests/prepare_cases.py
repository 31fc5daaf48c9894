"""Shared cases of the verifier's input preparation (TEST INFRASTRUCTURE, no GPU): IC = gamma_abc_g1[0] + sum_j x_j gamma_abc_g1[j + 1]
from a prepared key's window tables, tables[j][w][d - 1] = d * 16^w * gamma_abc_g1[j + 1].

The reference is pymodel's big-integer group law (pm.groups).  Keys are made from KNOWN discrete logarithms, gamma_abc_g1[j] = g_j G
(g_j = 0: the identity), so a point's expected value is one multiple of the generator and "two points are equal" is "their
logarithms are equal mod r".  chain() replays, on those logarithms, the partial sums prepare_inputs_tab forms -- bases in order,
windows from 0 upward -- and names what each table addition is for XYZZ::add_affine: an ordinary addition, the first point taken, a
doubling (the accumulator equals the entry) or a cancellation (it is the entry's negative).  tests/test_prepare_cases.py pins these
premises; the host and GPU tiers run the cases."""
import functools
import os
import re

import numpy as np

import pymodel as pm
from helpers import g1_to_arr, g2_to_arr, ints_to_mont

import groth16_amd as g
from groth16_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["bls12_381", "bn254"]
WINDOWS, DIGITS = 64, 15
NUM_PUBLIC = (0, 1, 2, 5, 33)


def source_constants():
    """the batch-shape constants of the verifier's sources, read from the text"""
    out = {}
    for path in ("verify_common.hpp", "verify_aggregate.hip"):
        text = open(os.path.join(ROOT, "groth16_amd", "csrc", path)).read()
        for name in ("VERIFY_BLOCK", "AGG_SCALAR_BLOCK", "AGG_MAX_PER_LANE", "WINDOWS", "DIGITS"):
            m = re.search(r"constexpr int [^;]*\b%s = (\d+)" % name, text)
            if m:
                out[name] = int(m.group(1))
    return out


def loop_order_in_source():
    """(bases in order, windows from 0 upward) as prepare_inputs_tab and tab_accumulate spell them: chain() replays THIS order, and
    the collision cases are derived for it"""
    text = open(os.path.join(ROOT, "groth16_amd", "csrc", "verify_common.hpp")).read()
    bases = "for (uint64_t j = 0; j < num_public; ++j) tab_accumulate<C>(acc, tables, j, x[j]);" in text
    windows = re.search(r"for \(int w = 0; w < WINDOWS; \+\+w\) \{\s*const uint32_t d = \(k\[w >> 3\] >> \(4 \* \(w & 7\)\)\) & 0xfu;\s*"
                        r"if \(d\) acc\.add_affine\(tables\[\(j \* WINDOWS \+ \(uint64_t\)w\) \* DIGITS \+ d - 1\]\);", text) is not None
    return bases, windows


# ---- scalars ------------------------------------------------------------------------------------------------------------------------
def top_nibble(r: int) -> int:
    return (r - 1) >> 252


def nibble(x: int, w: int) -> int:
    return (x >> (4 * w)) & 15


@functools.lru_cache(maxsize=None)
def scalar_list(curve: str):
    """the edge scalars of the issue, all below r, in a fixed order without repeats"""
    r = pm.CURVES[curve].r
    out = [0, 1, 2, 15, 16, 17, r - 1, r - 2, (r - 1) // 2]
    out += [sum(d << (4 * w) for w in range(WINDOWS - 1)) for d in range(1, DIGITS + 1)]
    out += [t << 252 for t in range(1, top_nibble(r) + 1)]
    for w in (1, 8, 9, 62, 63):
        out += [1 << (4 * w), (1 << (4 * w)) - 1]
    seen, uniq = set(), []
    for s in out:
        assert 0 <= s < r
        if s not in seen:
            seen.add(s)
            uniq.append(s)
    return tuple(uniq)


def reachable_entries(r: int):
    """every (w, d) some scalar below r selects"""
    return {(w, d) for w in range(WINDOWS - 1) for d in range(1, DIGITS + 1)} | {(WINDOWS - 1, d) for d in range(1, top_nibble(r) + 1)}


def selected_entries(scalars):
    return {(w, nibble(s, w)) for s in scalars for w in range(WINDOWS) if nibble(s, w)}


# ---- the model ----------------------------------------------------------------------------------------------------------------------
def model_table(cp, P):
    """[w][d - 1] = d * 16^w * P as affine points, by additions only (None throughout for the identity)"""
    G1 = pm.groups(cp)[0]
    rows, cur = [], P
    for _ in range(WINDOWS):
        row, acc = [], cur
        for _ in range(DIGITS):
            row.append(acc)
            acc = G1.add(acc, cur)
        rows.append(row)
        cur = acc   # 16 * cur
    return rows


@functools.lru_cache(maxsize=None)
def _generator_table(curve: str):
    cp = pm.CURVES[curve]
    G1 = pm.groups(cp)[0]
    return [[G1.to_jac(p) for p in row] for row in model_table(cp, cp.g1)]


@functools.lru_cache(maxsize=1 << 16)
def mul_g(curve: str, s: int):
    """s * G1 generator (affine, None for 0) from the generator's own model table"""
    cp = pm.CURVES[curve]
    G1 = pm.groups(cp)[0]
    s %= cp.r
    acc, tab = G1.jac_identity(), _generator_table(curve)
    for w in range(WINDOWS):
        d = nibble(s, w)
        if d:
            acc = G1.jadd(acc, tab[w][d - 1])
    return G1.to_affine(acc)


def fr_rows(curve: str, rows) -> np.ndarray:
    """rows of integers (ANY value below 2^256 is taken as given modulo r) -> uint64 [n, num_public, 4] Montgomery limbs"""
    r = pm.CURVES[curve].r
    rows = [list(row) for row in rows]
    m = len(rows[0]) if rows else 0
    flat = [v for row in rows for v in row]
    return ints_to_mont(flat, r, 4).reshape(len(rows), m, 4) if flat else np.zeros((len(rows), m, 4), np.uint64)


class CraftedKey:
    """a verifying key from known logarithms: gamma_abc_g1[j] = g[j] G, alpha G, beta G2, gamma G2, delta G2"""

    def __init__(self, curve, label, g_logs, seed=0x9E1, collision_rows=()):
        self.curve, self.label, self.cp = curve, label, pm.CURVES[curve]
        self.g = tuple(v % self.cp.r for v in g_logs)
        rng = pm.SplitMix64(seed + len(curve))
        self.alpha, self.beta, self.gamma, self.delta = (rng.field(self.cp.r - 1) + 1 for _ in range(4))
        self.collision_rows = tuple(collision_rows)   # [(row, [(j, w, kind)])]: events chain(row) must show
        self._vk = None

    def __repr__(self):
        return "%s/%s/%d" % (self.curve, self.label, self.num_public)

    @property
    def num_public(self):
        return len(self.g) - 1

    @property
    def points(self):
        return [mul_g(self.curve, v) for v in self.g]

    @property
    def vk(self):
        if self._vk is None:
            cp = self.cp
            G2 = pm.groups(cp)[1]
            self._vk = g.VerifyingKey(self.curve, g1_to_arr([mul_g(self.curve, self.alpha)], cp)[0],
                                      g2_to_arr([G2.mul(cp.g2, self.beta)], cp)[0], g2_to_arr([G2.mul(cp.g2, self.gamma)], cp)[0],
                                      g2_to_arr([G2.mul(cp.g2, self.delta)], cp)[0], g1_to_arr(self.points, cp))
        return self._vk

    def ic_log(self, row) -> int:
        assert len(row) == self.num_public
        return (self.g[0] + sum(x * gj for x, gj in zip(row, self.g[1:]))) % self.cp.r

    def expected_ic(self, row):
        return mul_g(self.curve, self.ic_log(row))

    def expected_ic_arr(self, rows) -> np.ndarray:
        return g1_to_arr([self.expected_ic(row) for row in rows], self.cp)

    def chain(self, row):
        """[(j, w, d, kind)] for every table addition prepare_inputs_tab makes on this row, in its order: kind is "add", "take" (the
        accumulator was the identity), "double" (it equals the entry) or "cancel" (it is the entry's negative).  An identity entry is
        skipped by add_affine before anything else and is not listed."""
        r = self.cp.r
        acc, out = self.g[0], []
        for j, x in enumerate(row):
            x %= r   # to_canonical reduces
            for w in range(WINDOWS):
                d = nibble(x, w)
                if not d or not self.g[j + 1]:
                    continue
                e = (d << (4 * w)) * self.g[j + 1] % r
                kind = "take" if acc == 0 else "double" if acc == e else "cancel" if (acc + e) % r == 0 else "add"
                out.append((j, w, d, kind))
                acc = (acc + e) % r
        assert acc == self.ic_log([x % r for x in row])
        return out

    # ---- proofs with an exact verdict
    def proof(self, row, k: int = 0):
        """A = a G1, B = b G2, C = c G1 with c = (a b - alpha beta - gamma ic) / delta: accepted exactly when the verifier forms
        ic = g_0 + sum x_j g_j.  k picks a and b.  Flat (A | B | C)."""
        return _proof(self, tuple(v % self.cp.r for v in row), k)


@functools.lru_cache(maxsize=None)
def _b_g2(curve: str, b: int):
    cp = pm.CURVES[curve]
    return g2_to_arr([pm.groups(cp)[1].mul(cp.g2, b)], cp)[0]


@functools.lru_cache(maxsize=None)
def _proof(key: CraftedKey, row, k: int):
    cp, r = key.cp, key.cp.r
    rng = pm.SplitMix64(0xAB0 + k)
    a, b = rng.field(r - 1) + 1, 0xB0B + (k % 3)   # few distinct B: a G2 multiple is the model's slowest step
    c = (a * b - key.alpha * key.beta - key.gamma * key.ic_log(row)) * pow(key.delta, -1, r) % r
    return np.concatenate([g1_to_arr([mul_g(key.curve, a)], cp)[0], _b_g2(key.curve, b), g1_to_arr([mul_g(key.curve, c)], cp)[0]])


def bump(row, j: int, r: int):
    """the row with x_j replaced by x_j + 1"""
    out = list(row)
    out[j] = (out[j] + 1) % r
    return tuple(out)


def live_input(key, j: int) -> int:
    """the first input at or after j (cyclically) whose base is not the identity: changing it changes IC"""
    m = key.num_public
    return next(k % m for k in range(j, j + m) if key.g[k % m + 1])


# ---- keys ---------------------------------------------------------------------------------------------------------------------------
def _logs(curve: str, seed: int, n: int):
    r = pm.CURVES[curve].r
    rng = pm.SplitMix64(seed)
    return [rng.field(r - 1) + 1 for _ in range(n)]


@functools.lru_cache(maxsize=None)
def key_random(curve: str, num_public: int) -> CraftedKey:
    """(a)"""
    return CraftedKey(curve, "a_random", _logs(curve, 0xA0 + num_public, num_public + 1))


@functools.lru_cache(maxsize=None)
def key_identity_first(curve: str, num_public: int = 5) -> CraftedKey:
    """(b): gamma_abc_g1[0] is the identity"""
    return CraftedKey(curve, "b_identity_at_0", [0] + _logs(curve, 0xB0 + num_public, num_public))


@functools.lru_cache(maxsize=None)
def key_identity_inside(curve: str, num_public: int = 5) -> CraftedKey:
    """(c): an identity at j = 3 (j = 1 for a single input), live bases beside it"""
    logs = _logs(curve, 0xC0 + num_public, num_public + 1)
    logs[min(3, num_public)] = 0
    return CraftedKey(curve, "c_identity_inside", logs)


@functools.lru_cache(maxsize=None)
def key_equal_bases(curve: str) -> CraftedKey:
    """(d): g_1 = g_2 and gamma_abc_g1[0] the identity, five inputs.  With x_1 = x_2 = 9 * 16^5 the first base leaves the accumulator
    at x_1 g_1 and the second base's only entry is that very point: a doubling.  With x_2 = r - x_1 the accumulator runs through
    (x_1 + the low windows of r - x_1) g_1 and meets the negative of the LAST entry of base 2: a cancellation, at the top window.
    Bases 3 .. 5 follow with ordinary inputs."""
    r = pm.CURVES[curve].r
    a, *rest = _logs(curve, 0xD0, 4)
    x = 9 << 20
    tail = tuple(_logs(curve, 0xD1, 3))
    w_top = max(w for w in range(WINDOWS) if nibble(r - x, w))
    rows = [((x, x) + tail, [(1, 5, "double")]), ((x, r - x) + tail, [(1, w_top, "cancel")])]
    return CraftedKey(curve, "d_equal_bases", [0, a, a] + rest, collision_rows=rows)


def collision_entries(curve: str):
    return [(0, 1), (5, 15), (WINDOWS - 1, top_nibble(pm.CURVES[curve].r))]


@functools.lru_cache(maxsize=None)
def key_first_addition(curve: str, w: int, d: int, sign: int) -> CraftedKey:
    """(e): g_0 = sign * d * 16^w * g_1, two inputs.  x_1 has zero windows below w, the digit d at w and live windows above it (none
    above w = 63: base 2 follows instead), so the FIRST addition from the tables is a doubling (sign = +1) or a cancellation to the
    identity (sign = -1, the next addition then takes its entry), and ordinary additions follow."""
    r = pm.CURVES[curve].r
    a, b = _logs(curve, 0xE0 + w, 2)
    high = 0
    if w < WINDOWS - 1:
        rng = pm.SplitMix64(0xE1 + w)
        high = (rng.field(1 << 248) >> (4 * (w + 1))) << (4 * (w + 1))   # below 2^248 < r, nothing at or below window w
    x1 = (d << (4 * w)) + high
    assert x1 < r and nibble(x1, w) == d and x1 % (1 << (4 * w)) == 0
    x2 = _logs(curve, 0xE2 + w, 1)[0]
    kind = "double" if sign > 0 else "cancel"
    return CraftedKey(curve, "e_first_%s_w%d_d%d" % (kind, w, d), [sign * (d << (4 * w)) * a, a, b], collision_rows=[((x1, x2), [(0, w, kind)])])


@functools.lru_cache(maxsize=None)
def key_identity_ic(curve: str) -> CraftedKey:
    """(f): five inputs whose IC is the identity although no term is (identity_ic_case with five inputs): x_5 solves
    g_0 + sum x_j g_j = 0, so the last addition of base 5 cancels"""
    r = pm.CURVES[curve].r
    logs = _logs(curve, 0xF0, 6)
    xs = _logs(curve, 0xF1, 4)
    x5 = -(logs[0] + sum(x * gj for x, gj in zip(xs, logs[1:5]))) * pow(logs[5], -1, r) % r
    w_top = max(w for w in range(WINDOWS) if nibble(x5, w))
    return CraftedKey(curve, "f_identity_ic", logs, collision_rows=[(tuple(xs) + (x5,), [(4, w_top, "cancel")])])


def collision_keys(curve: str):
    out = [key_equal_bases(curve)]
    for w, d in collision_entries(curve):
        out += [key_first_addition(curve, w, d, +1), key_first_addition(curve, w, d, -1)]
    return out + [key_identity_ic(curve)]


def table_keys(curve: str, sizes=(1, 5)):
    """keys (a) to (c) at the given input counts"""
    return [mk(curve, m) for m in sizes for mk in (key_random, key_identity_first, key_identity_inside)]


def all_keys(curve: str):
    return [key_random(curve, m) for m in NUM_PUBLIC] + [key_identity_first(curve), key_identity_inside(curve)] + collision_keys(curve)


def rows_for(key: CraftedKey, n: int):
    """n input rows, all different for two inputs or more (for one input: while the scalar list lasts): row i takes the scalar list
    from position i with a step per input that grows each time the list wraps, and the key's collision rows sit at lanes 0, 7, 14 ...:
    a wave then mixes zero inputs, r - 1, collision rows and ordinary rows"""
    S, m = scalar_list(key.curve), key.num_public
    special = [row for row, _ in key.collision_rows]
    rows = []
    for i in range(n):
        if special and i % 7 == 0 and i // 7 < len(special):
            rows.append(tuple(special[i // 7]))
        else:
            rows.append(tuple(S[(i + (5 + i // len(S)) * j) % len(S)] for j in range(m)))
    return rows


# ---- unreduced input words ----------------------------------------------------------------------------------------------------------
def unreduced_rows(curve: str, values):
    """(uint64 [n, 1, 4] rows, the values to_canonical yields): the Montgomery words of each value PLUS r -- 256 bits suffice on both
    curves -- and one row of all-ones words"""
    r = pm.CURVES[curve].r
    R = 1 << 256
    words, reduced = [], []
    for v in values:
        m = (v % r) * R % r + r
        assert r <= m < R
        words.append(m)
        reduced.append(v % r)
    words.append(R - 1)
    reduced.append((R - 1) * pow(R, -1, r) % r)
    arr = np.array([[[(m >> (64 * k)) & (2**64 - 1) for k in range(4)]] for m in words], dtype=np.uint64)
    return arr, reduced


# ---- verdict batches ----------------------------------------------------------------------------------------------------------------
def coefficients(n: int, seed: int = 0xC0EF):
    """n fixed non-zero 128-bit coefficients: the aggregate calls are then deterministic and equal their host twins'"""
    rng = pm.SplitMix64(seed)
    return [((rng.next() << 64) | rng.next()) | 1 for _ in range(n)]


def verdict_batch(key: CraftedKey, n: int, alter=None):
    """(flat proofs [n], input rows uint64 [n, num_public, 4]): proof i is exact for row i, the rows cycling through rows_for(key, 8)
    (collision rows included).  alter = i: in row i one input on a live base (live_input(key, i)) becomes x + 1 and the proof stays --
    that proof is then rejected, every other one still accepted."""
    base = rows_for(key, 8)
    rows = [base[i % 8] for i in range(n)]
    proofs = [key.proof(base[i % 8], i % 8) for i in range(n)]
    if alter is not None:
        assert key.num_public
        rows[alter] = bump(rows[alter], live_input(key, alter), key.cp.r)
    return proofs, fr_rows(key.curve, rows)


def alter_positions(n: int):
    return sorted({0, n // 2, n - 1})


def mixed_batch(keys, n: int, alter=None):
    """(key_of, proofs, ragged input rows): proof i under keys[i mod len(keys)], exact for its row; alter as verdict_batch"""
    key_of, proofs, rows = [], [], []
    for i in range(n):
        key = keys[i % len(keys)]
        row = rows_for(key, 8)[(i // len(keys)) % 8]
        proofs.append(key.proof(row, (i // len(keys)) % 8))
        if alter == i:
            assert key.num_public
            row = bump(row, live_input(key, i), key.cp.r)
        key_of.append(i % len(keys))
        rows.append(fr_rows(key.curve, [row])[0])
    return key_of, proofs, rows


def unreduced_case(curve: str):
    """key (a) with one input; rows whose words are x + r (and one all-ones row); per row a proof exact at the value to_canonical
    yields (the model's verdict: 1) and one exact at that value + 1 (the model's verdict: 0).
    Returns (key, rows uint64 [n, 1, 4], reduced values, honest proofs, wrong proofs)."""
    key = key_random(curve, 1)
    r = key.cp.r
    rows, reduced = unreduced_rows(curve, [0, 1, r - 1, scalar_list(curve)[9], 0xFEEDFACE << 190])
    honest = [key.proof((v,), k) for k, v in enumerate(reduced)]
    wrong = [key.proof(((v + 1) % r,), k) for k, v in enumerate(reduced)]
    return key, rows, reduced, honest, wrong


# ---- the host twins and the model's tables, as arrays ------------------------------------------------------------------------------
N_KEYS = 15   # all_keys: (a) at five input counts, (b), (c), the eight collision keys
FILL = 0xDEADBEEFDEADBEEF


def host_tables(key):
    view, keep = key.vk.view()
    st, tab = binding.host_pvk_tables(g.lib(), binding.CURVE_ID[key.curve], view, key.num_public, binding.FQ_LIMBS[key.curve])
    assert st == 0
    return tab


def host_ic(key, rows_arr):
    view, keep = key.vk.view()
    st, ic = binding.host_prepare_inputs(g.lib(), binding.CURVE_ID[key.curve], view, rows_arr, key.num_public, binding.FQ_LIMBS[key.curve])
    assert st == 0
    return ic


def model_tables(key, bases=None):
    """uint64 [len(bases), 64, 15, 2 L] for the listed bases (all by default)"""
    cp = key.cp
    bases = range(key.num_public) if bases is None else bases
    return np.stack([g1_to_arr([p for row in model_table(cp, key.points[j + 1]) for p in row], cp).reshape(WINDOWS, DIGITS, -1)
                     for j in bases])
