#!/usr/bin/env python3
"""Generates params_gen.hpp: Montgomery constants (32-bit limbs, R = 2^(32N) which equals
arkworks' R = 2^(64*N/2)) for the two curves the prover supports.  Run by
__graft_entry__.build() / the Makefile; output is committed so the GPU box needs no step.

Constants: BLS12-381 and BN254 field moduli, Fr multiplicative generator and 2-adicity
(ark-bls12-381 / ark-bn254 0.5.0 Fr configs: GENERATOR = 7 / 5, TWO_ADICITY = 32 / 28),
curve coefficients and standard generators.

Pairing constants (pairing.hpp), in the 30-bit Montgomery form the pairing arithmetic runs in (x * 2^(30 NL) mod q):
the sextic non-residue xi = s + u (Fq6 = Fq2[v]/(v^3 - xi), Fq12 = Fq6[w]/(w^2 - v), so w^6 = xi), the Frobenius
coefficients gamma[j][k] = xi^(k (q^j - 1) / 6) that map a w^k coefficient under the j-th power of Frobenius (j = 1..3,
k = 1..5: Fq6 = even k, Fq12 = odd k; Fq2's own Frobenius is conjugation), 1/2, and the loop parameters: BLS12-381
|x| with x negative, BN254 6x + 2 as non-adjacent signed digits and x for the final exponentiation.

Membership constants (subgroup.hpp): BLS12-381 beta (G1's endomorphism) and psi's two coefficients on the M-type twist,
BN254 6x^2 (psi's eigenvalue on G2).
"""
import os

CURVES = {
    "Bls12_381": dict(
        q=0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB,
        r=0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001,
        gen=7, s=32, b1=4, b2=(4, 4), xi=1, x=-0xD201000000010000,
        g1=(0x17F1D3A73197D7942695638C4FA9AC0FC3688C4F9774B905A14E3A3F171BAC586C55E83FF97A1AEFFB3AF00ADB22C6BB,
            0x08B3F481E3AAA0F1A09E30ED741D8AE4FCF5E095D5D00AF600DB18CB2C04B3EDD03CC744A2888AE40CAA232946C5E7E1),
        g2=(0x024AA2B2F08F0A91260805272DC51051C6E47AD4FA403B02B4510B647AE3D1770BAC0326A805BBEFD48056C8C121BDB8,
            0x13E02B6052719F607DACD3A088274F65596BD0D09920B61AB5DA61BBDC7F5049334CF11213945D57E5AC7D055D042B7E,
            0x0CE5D527727D6E118CC9CDC6DA2E351AADFD9BAA8CBDD3A76D429A695160D12C923AC9CC3BACA289E193548608B82801,
            0x0606C4A02EA734CC32ACD2B02BC28B99CB3E287E85A763AF267492AB572E99AB3F370D275CEC1DA1AAA9075FF05F79BE),
    ),
    "Bn254": dict(
        q=21888242871839275222246405745257275088696311157297823662689037894645226208583,
        r=21888242871839275222246405745257275088548364400416034343698204186575808495617,
        gen=5, s=28, b1=3, b2=None,  # 3/(9+u), computed below
        xi=9, x=4965661367192848881,
        g1=(1, 2),
        g2=(10857046999023057135944570762232829481370756359578518086990519993285655852781,
            11559732032986387107991004021392285783925812861821192530917403151452391805634,
            8495653923123431417604973247489272438418190587263600148770280649306958101930,
            4082367875863433681332203403145435568316851327593401208105741076214120093531),
    ),
}


def limbs32(v, n):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def arr(vals):
    return "{" + ", ".join("0x%08xu" % v for v in vals) + "}"


def field_struct(name, p):
    n = (p.bit_length() + 31) // 32
    if n % 2:
        n += 1  # keep 64-bit limb compatibility
    R = 1 << (32 * n)
    inv = (-pow(p, -1, 1 << 32)) % (1 << 32)
    out = []
    out.append("struct %s {" % name)
    out.append("    static constexpr int N = %d;" % n)
    out.append("    static constexpr int BITS = %d;" % p.bit_length())
    out.append("    static constexpr uint32_t INV = 0x%08xu;  // -p^-1 mod 2^32" % inv)
    for fn, val in (("mod", p), ("r1", R % p), ("r2", R * R % p), ("pm2", p - 2)):
        out.append("    G16_HD static constexpr uint32_t %s(int i) {" % fn)
        out.append("        constexpr uint32_t t[N] = %s;" % arr(limbs32(val, n)))
        out.append("        return t[i];")
        out.append("    }")
    # ---- 30-bit reduced-radix view (fp30.hpp): NL limbs, R' = 2^(30 NL)
    nl = (p.bit_length() + 29) // 30
    R30 = 1 << (30 * nl)
    M30 = (1 << 30) - 1

    def limbs30(v, cnt=nl):
        return [(v >> (30 * i)) & M30 for i in range(cnt - 1)] + [v >> (30 * (cnt - 1))]

    def redundant(k):  # k*p with every limb but the top >= 2^30 - 1, so limb-wise a + KP - b never borrows
        l = limbs30(k * p)
        r = [l[0] + (1 << 30)] + [x + (1 << 30) - 1 for x in l[1:-1]] + [l[-1] - 1]
        assert sum(x << (30 * i) for i, x in enumerate(r)) == k * p
        return r

    out.append("    static constexpr int NL30 = %d;" % nl)
    out.append("    static constexpr uint32_t PINV30 = 0x%08xu;   // -p^-1 mod 2^30" % ((-pow(p, -1, 1 << 30)) % (1 << 30)))
    out.append("    static constexpr uint32_t PPINV30 = 0x%08xu;  //  p^-1 mod 2^30" % (pow(p, -1, 1 << 30)))
    for fn, vals in (("p30", limbs30(p)), ("one30", limbs30(R30 % p)), ("rstd30", limbs30(R % p)), ("r3_30", limbs30(pow(R30, 3, p))), ("kp2", redundant(2)),
                     ("kp4", redundant(4)), ("kp6", redundant(6)), ("kp8", redundant(8)), ("kp16", redundant(16)), ("np2", limbs30(2 * p)),
                     ("np4", limbs30(4 * p)), ("np8", limbs30(8 * p)), ("np16", limbs30(16 * p))):
        out.append("    G16_HD static constexpr uint32_t %s(int i) {" % fn)
        out.append("        constexpr uint32_t t[NL30] = %s;" % arr(vals))
        out.append("        return t[i];")
        out.append("    }")
    # redundant 2^(k+1) * p for k = 0..11 (lazy DIF butterflies subtract operands that double every stage)
    if name.endswith("FrP"):   # scalar fields only (the NTT); their top limb has room for 4096 p
        out.append("    G16_HD static constexpr uint32_t kp_pow2(int k, int i) {")
        out.append("        constexpr uint32_t t[12][NL30] = {%s};" % ", ".join(arr(redundant(2 << k)) for k in range(12)))
        out.append("        return t[k][i];")
        out.append("    }")
    # 2^(30 NL) mod p as a plain integer in 32-bit limbs: std-Montgomery multiplying x*R by it gives x*R' mod p
    out.append("    G16_HD static constexpr uint32_t r30_plain(int i) {")
    out.append("        constexpr uint32_t t[N] = %s;" % arr(limbs32(R30 % p, n)))
    out.append("        return t[i];")
    out.append("    }")
    out.append("};")
    return "\n".join(out), n, R


def limbs30_of(v, p):
    nl = (p.bit_length() + 29) // 30
    return [(v >> (30 * i)) & ((1 << 30) - 1) for i in range(nl - 1)] + [v >> (30 * (nl - 1))]


def mont30(v, p):
    nl = (p.bit_length() + 29) // 30
    return limbs30_of(v % p * (1 << (30 * nl)) % p, p)


def fq2_mul(a, b, q):
    return ((a[0] * b[0] - a[1] * b[1]) % q, (a[0] * b[1] + a[1] * b[0]) % q)


def fq2_pow(a, e, q):
    r = (1, 0)
    for bit in bin(e)[2:]:
        r = fq2_mul(r, r, q)
        if bit == "1":
            r = fq2_mul(r, a, q)
    return r


def naf(n):
    out = []
    while n:
        if n & 1:
            d = 2 - (n & 3)
            n -= d
        else:
            d = 0
        out.append(d)
        n >>= 1
    return out  # little-endian digits in {-1, 0, 1}


def fq2_inv(a, q):
    n = pow((a[0] * a[0] + a[1] * a[1]) % q, q - 2, q)
    return (a[0] * n % q, -a[1] * n % q)


def ec_add(P, Q, q):
    """affine addition on y^2 = x^3 + b over Fq2 (Fq embeds as (a, 0)); None is the identity"""
    if P is None:
        return Q
    if Q is None:
        return P
    sub = lambda a, b: ((a[0] - b[0]) % q, (a[1] - b[1]) % q)
    if P[0] == Q[0]:
        if P[1] != Q[1] or P[1] == (0, 0):
            return None
        x2 = fq2_mul(P[0], P[0], q)
        lam = fq2_mul(((3 * x2[0]) % q, (3 * x2[1]) % q), fq2_inv(((2 * P[1][0]) % q, (2 * P[1][1]) % q), q), q)
    else:
        lam = fq2_mul(sub(Q[1], P[1]), fq2_inv(sub(Q[0], P[0]), q), q)
    x3 = sub(sub(fq2_mul(lam, lam, q), P[0]), Q[0])
    return (x3, sub(fq2_mul(lam, sub(P[0], x3), q), P[1]))


def ec_mul(P, k, q):
    acc = None
    for bit in bin(k)[2:]:
        acc = ec_add(acc, acc, q)
        if bit == "1":
            acc = ec_add(acc, P, q)
    return acc


def subgroup_consts(c):
    """lines of the Consts struct that subgroup.hpp reads: the endomorphism constants of the membership tests, each checked
    here against a big-int scalar multiple of the generator (so the right root is chosen now, not by trial at run time)"""
    q, r, x, xi = c["q"], c["r"], c["x"], (c["xi"], 1)
    nl = (q.bit_length() + 29) // 30
    conj = lambda a: (a[0], -a[1] % q)
    g1 = ((c["g1"][0], 0), (c["g1"][1], 0))
    g2 = ((c["g2"][0], c["g2"][1]), (c["g2"][2], c["g2"][3]))
    o = []

    def emit(name, rows):
        o.append("    G16_HD static constexpr uint32_t %s(int k, int i) {" % name)
        o.append("        constexpr uint32_t t[%d][%d] = {%s};" % (len(rows), nl, ", ".join(arr(mont30(v, q)) for v in rows)))
        o.append("        return t[k][i];")
        o.append("    }")

    if c["xi"] == 1:
        # G1: phi(x, y) = (beta x, y) acts on the r-torsion as -x^2 (a root of l^2 + l + 1 mod r = x^4 - x^2 + 1)
        assert r == x ** 4 - x ** 2 + 1
        g = 2
        while pow(g, (q - 1) // 3, q) == 1:
            g += 1
        b = pow(g, (q - 1) // 3, q)
        want = ec_mul(g1, (-x * x) % r, q)
        beta = [v for v in (b, b * b % q) if ((v * g1[0][0] % q, 0), g1[1]) == want]
        assert len(beta) == 1 and pow(beta[0], 3, q) == 1 and beta[0] != 1
        o.append("    // beta: the cube root of unity with (beta x, y) = -[x^2](x, y) on G1; 30-bit Montgomery form")
        emit("endo_beta30", beta)
        # G2: psi = twist o Frobenius o untwist on the M-type twist, (conj(x) cx, conj(y) cy), acts as x
        cx, cy = fq2_inv(fq2_pow(xi, (q - 1) // 3, q), q), fq2_inv(fq2_pow(xi, (q - 1) // 2, q), q)
        scalar = x % r
    else:
        # G1 has cofactor 1.  G2: psi on the D-type twist is pairing.hpp's frob_twist(q, 1) and acts as q = 6x^2 mod r
        assert q + 1 - (6 * x * x + 1) == r
        cx, cy = fq2_pow(xi, (q - 1) // 3, q), fq2_pow(xi, (q - 1) // 2, q)
        scalar = 6 * x * x
        assert scalar.bit_length() == 127
        o.append("    static constexpr uint64_t G2_ENDO_LO = 0x%016xull, G2_ENDO_HI = 0x%016xull;  // 6x^2, psi's eigenvalue on G2"
                 % (scalar & (2 ** 64 - 1), scalar >> 64))
    assert (fq2_mul(conj(g2[0]), cx, q), fq2_mul(conj(g2[1]), cy, q)) == ec_mul(g2, scalar, q)
    if c["xi"] == 1:
        o.append("    // psi(x, y) = (conj(x) psi[0..1], conj(y) psi[2..3]) = [x](x, y) on G2: xi^(-(q-1)/3), xi^(-(q-1)/2)")
        emit("psi30", [cx[0], cx[1], cy[0], cy[1]])
    return o


def pairing_consts(c):
    """lines of the Consts struct that pairing.hpp reads"""
    q, xi, x = c["q"], (c["xi"], 1), c["x"]
    nl = (q.bit_length() + 29) // 30
    o = []
    o.append("    static constexpr int XI = %d;  // xi = XI + u" % c["xi"])
    gam = []
    for j in (1, 2, 3):
        for k in range(1, 6):
            g = fq2_pow(xi, k * (q ** j - 1) // 6, q)
            gam.append(mont30(g[0], q))
            gam.append(mont30(g[1], q))
    o.append("    // gamma[j-1][k-1][c] = component c of xi^(k (q^j - 1) / 6), 30-bit Montgomery form")
    o.append("    G16_HD static constexpr uint32_t frob30(int j, int k, int c, int i) {")
    o.append("        constexpr uint32_t t[30][%d] = {%s};" % (nl, ", ".join(arr(g) for g in gam)))
    o.append("        return t[((j - 1) * 5 + (k - 1)) * 2 + c][i];")
    o.append("    }")
    o.append("    G16_HD static constexpr uint32_t two_inv30(int i) {")
    o.append("        constexpr uint32_t t[%d] = %s;" % (nl, arr(mont30(pow(2, q - 2, q), q))))
    o.append("        return t[i];")
    o.append("    }")
    o.append("    static constexpr uint64_t ATE_X_ABS = 0x%016xull;" % abs(x))
    o.append("    static constexpr bool ATE_X_NEG = %s;" % ("true" if x < 0 else "false"))
    if c["xi"] == 1:
        # BLS12: the Miller loop runs over |x|; the hard part of the final exponentiation uses (x - 1)^2 / 3
        assert (x - 1) ** 2 % 3 == 0
        e = (x - 1) ** 2 // 3
        o.append("    static constexpr uint64_t HARD_E_LO = 0x%016xull, HARD_E_HI = 0x%016xull;  // (x - 1)^2 / 3" % (e & (2 ** 64 - 1), e >> 64))
        o.append("    static constexpr int ATE_NAF_LEN = 0;")
        o.append("    G16_HD static constexpr int ate_naf(int) { return 0; }")
    else:
        d = naf(6 * x + 2)
        assert sum(v << i for i, v in enumerate(d)) == 6 * x + 2
        o.append("    static constexpr uint64_t HARD_E_LO = 0, HARD_E_HI = 0;")
        o.append("    static constexpr int ATE_NAF_LEN = %d;  // non-adjacent form of 6x + 2, little-endian" % len(d))
        o.append("    G16_HD static constexpr int ate_naf(int i) {")
        o.append("        constexpr signed char t[%d] = {%s};" % (len(d), ", ".join(str(v) for v in d)))
        o.append("        return t[i];")
        o.append("    }")
    return o


def mont(v, p, R, n):
    return arr(limbs32(v % p * R % p, n))


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    o = []
    o.append("// GENERATED by gen_params.py -- do not edit.")
    o.append("#pragma once")
    o.append("#include <cstdint>")
    o.append('#include "hd.hpp"')
    o.append("namespace g16 {")
    for cname, c in CURVES.items():
        q, r = c["q"], c["r"]
        fq_s, nq, Rq = field_struct(cname + "FqP", q)
        fr_s, nr, Rr = field_struct(cname + "FrP", r)
        o.append(fq_s)
        o.append(fr_s)
        root = pow(c["gen"], (r - 1) >> c["s"], r)
        b2 = c["b2"]
        if b2 is None:
            # 3 / (9 + u) in Fq[u]/(u^2+1):  3 * (9 - u) / 82
            inv82 = pow(82, q - 2, q)
            b2 = (27 * inv82 % q, (-3) * inv82 % q)
        o.append("struct %sConsts {" % cname)
        o.append("    static constexpr int TWO_ADICITY = %d;" % c["s"])
        for nm, val, p, R, n in (
            ("fr_generator", c["gen"], r, Rr, nr), ("fr_generator_inv", pow(c["gen"], r - 2, r), r, Rr, nr),
            ("two_adic_root", root, r, Rr, nr),
            ("b1", c["b1"], q, Rq, nq), ("b2_c0", b2[0], q, Rq, nq), ("b2_c1", b2[1], q, Rq, nq),
            ("g1_x", c["g1"][0], q, Rq, nq), ("g1_y", c["g1"][1], q, Rq, nq),
            ("g2_x0", c["g2"][0], q, Rq, nq), ("g2_x1", c["g2"][1], q, Rq, nq),
            ("g2_y0", c["g2"][2], q, Rq, nq), ("g2_y1", c["g2"][3], q, Rq, nq),
        ):
            o.append("    G16_HD static constexpr uint32_t %s(int i) {" % nm)
            o.append("        constexpr uint32_t t[%d] = %s;" % (n, mont(val, p, R, n)))
            o.append("        return t[i];")
            o.append("    }")
        o.extend(pairing_consts(c))
        o.extend(subgroup_consts(c))
        o.append("};")
    o.append("}  // namespace g16")
    with open(os.path.join(here, "params_gen.hpp"), "w") as f:
        f.write("\n".join(o) + "\n")


if __name__ == "__main__":
    main()
