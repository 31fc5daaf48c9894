"""Test-side big-int model of the optimal-ate pairing the library computes (groth16_amd/csrc/pairing.hpp): BLS12-381 and BN254.

Independent of the library's formulas: the Miller loop runs on the untwisted points in E(Fq12) with affine lines (pymodel's
Fq12 = Fq[w]/(w^12 - c6 w^6 - c0) and `untwist`), keeping T on the twist only to get the slope cheaply; the final exponentiation
is a plain pow by (q^12 - 1) / r.  Results are converted to arkworks' tower order (Fq6 = Fq2[v]/(v^3 - xi), Fq12 = Fq6[w]/(w^2 -
v)) so they compare with the library's GT bytes.  About a second per pairing."""
from functools import lru_cache

import pymodel as pm

LOOP = {"bls12_381": dict(x=-0xD201000000010000), "bn254": dict(x=4965661367192848881)}


@lru_cache(maxsize=None)
def _ctx(name):
    cp = pm.CURVES[name]
    F = pm.Fq12(cp)
    w = [0, 1] + [0] * 10
    w2, w3 = F.mul(w, w), F.mul(w, F.mul(w, w))
    winv = F.inv(w)
    return cp, F, w, winv, w2, w3, F.mul(winv, winv), F.mul(winv, F.mul(winv, winv))


def _untwist(name, Q):
    cp, F, w, winv, w2, w3, wi2, wi3 = _ctx(name)
    x, y = F.from_fq2(Q[0]), F.from_fq2(Q[1])
    if pm._TOWER[name]["twist"] == "D":
        return F.mul(x, w2), F.mul(y, w3)
    return F.mul(x, wi2), F.mul(y, wi3)


def _line(name, T, lam2, P):
    """l(P) = yP - yT - lam (xP - xT) for the line through the untwisted T with twist slope lam2 (lam = lam2 * w^(+-1))"""
    cp, F, w, winv, *_ = _ctx(name)
    xt, yt = _untwist(name, T)
    lam = F.mul(F.from_fq2(lam2), w if pm._TOWER[name]["twist"] == "D" else winv)
    xp = [P[0]] + [0] * 11
    yp = [P[1]] + [0] * 11
    return F.sub(F.sub(yp, yt), F.mul(lam, F.sub(xp, xt)))


def _step(name, T, R, P):
    """(line through T and R (tangent if equal) at P, T + R) on the twist; None for a vertical line (its value lies in a
    subfield that the final exponentiation kills)"""
    cp = pm.CURVES[name]
    F2 = pm.Fq2(cp.q)
    if T[0] == R[0]:
        if F2.add(T[1], R[1]) == F2.zero:
            return None, None
        lam = F2.mul(F2.mul(F2.from_int(3), F2.sqr(T[0])), F2.inv(F2.add(T[1], T[1])))
    else:
        lam = F2.mul(F2.sub(R[1], T[1]), F2.inv(F2.sub(R[0], T[0])))
    x3 = F2.sub(F2.sub(F2.sqr(lam), T[0]), R[0])
    y3 = F2.sub(F2.mul(lam, F2.sub(T[0], x3)), T[1])
    return _line(name, T, lam, P), (x3, y3)


def _frob_twist(name, Q, k):
    """pi^k(Q) expressed on the (D-type) twist, from xi^((q^k - 1)/3) and xi^((q^k - 1)/2)"""
    cp = pm.CURVES[name]
    F2 = pm.Fq2(cp.q)
    xi = (pm._TOWER[name]["s"], 1)

    def pw(a, e):
        r = F2.one
        for bit in bin(e)[2:]:
            r = F2.mul(r, r)
            if bit == "1":
                r = F2.mul(r, a)
        return r

    x, y = Q
    if k & 1:
        x, y = (x[0], (-x[1]) % cp.q), (y[0], (-y[1]) % cp.q)
    return F2.mul(x, pw(xi, (cp.q ** k - 1) // 3)), F2.mul(y, pw(xi, (cp.q ** k - 1) // 2))


def miller_loop(name, P, Q):
    cp, F, *_ = _ctx(name)
    if P is None or Q is None:
        return F.one
    x = LOOP[name]["x"]
    n = abs(x) if name == "bls12_381" else 6 * x + 2
    f, T = F.one, Q
    for bit in bin(n)[3:]:
        l, T = _step(name, T, T, P)
        f = F.mul(F.mul(f, f), l)
        if bit == "1":
            l, T = _step(name, T, Q, P)
            f = F.mul(f, l)
    if name == "bls12_381":
        return F.pow(f, cp.q ** 6) if x < 0 else f   # conjugation = the q^6-th power
    q1 = _frob_twist(name, Q, 1)
    q2 = _frob_twist(name, Q, 2)
    q2 = (q2[0], ((-q2[1][0]) % cp.q, (-q2[1][1]) % cp.q))
    l, T = _step(name, T, q1, P)
    f = F.mul(f, l)
    l, T = _step(name, T, q2, P)
    if l is not None:
        f = F.mul(f, l)
    return f


def final_exponentiation(name, f):
    cp, F, *_ = _ctx(name)
    return F.pow(f, (cp.q ** 12 - 1) // cp.r)


def pairing(name, P, Q):
    return final_exponentiation(name, miller_loop(name, P, Q))


def pairing_product(name, pairs):
    cp, F, *_ = _ctx(name)
    f = F.one
    for P, Q in pairs:
        f = F.mul(f, miller_loop(name, P, Q))
    return final_exponentiation(name, f)


def to_ark(name, a):
    """pymodel Fq12 (12 Fq coefficients of w^k, u = w^6 - s) -> arkworks' 12 Fq in c0.c0.c0 ... c1.c2.c1 order (integers)"""
    cp = pm.CURVES[name]
    s = pm._TOWER[name]["s"]
    coef = [((a[k] + s * a[k + 6]) % cp.q, a[k + 6] % cp.q) for k in range(6)]   # Fq2 coefficient of w^k
    out = []
    for k in (0, 2, 4, 1, 3, 5):   # c0 = (w^0, w^2, w^4), c1 = (w^1, w^3, w^5)
        out.extend(coef[k])
    return out


def to_ark_limbs(name, a):
    import numpy as np

    cp = pm.CURVES[name]
    return np.array([l for v in to_ark(name, a) for l in pm.to_mont_limbs(v, cp.q, cp.fq_limbs64)], dtype=np.uint64)
