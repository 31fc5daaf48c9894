"""Literal big-int model of the Circom R1CS -> QAP reduction (TEST INFRASTRUCTURE; shares no code with the library).

Restated from the published source of ark-circom's CircomReduction; not pinned against it (it is not available here).  What
pins it instead is in test_circom_host.py: the algebraic identity that ties its h to the Libsnark map's, and the identity
sum_k h[k] s[k] = delta^-1 (A B - C)(t) that ties its two functions to each other.

F = Fr, n = the power of two >= num_constraints + num_inputs, w = the n-th root the transforms use, rho = the generator of
the 2n-point radix-2 domain (rho^2 = w).

witness_map(cp, cs, z):
  1. rows i < nc: a[i] = <A_i, z>, b[i] = <B_i, z>; rows nc <= i < nc + ni: a[i] = z[i - nc], b[i] = 0; 0 above
  2. c[i] = a[i] b[i]     (the C matrix is not read)
  3. each of a, b, c: inverse transform on the domain, element i times rho^i, forward transform
  4. h[i] = a[i] b[i] - c[i], n values, natural order

h_query_scalars(cp, n, t, delta_inv):
  the 2n - 1 values delta^-1 t^i zero-padded to 2n, inverse transform of size 2n (out[j] = (2n)^-1 sum_i v_i rho^(-ij)),
  the odd-indexed entries -- n scalars.

The transforms are plain DFT sums up to 32 points and pymodel's radix-2 recursion above (DFT_SUM_LIMIT; test_circom_host
checks the two against each other at the limit)."""
import pymodel as pm

DFT_SUM_LIMIT = 32


def roots(cp, n):
    """(w, rho): the generators of the n-point and the 2n-point domain, both from the field's two-adic root"""
    log_n = n.bit_length() - 1
    assert 1 << log_n == n
    if log_n + 1 > cp.two_adicity:
        raise ValueError("PolynomialDegreeTooLarge")
    rho = cp.two_adic_root
    for _ in range(cp.two_adicity - log_n - 1):
        rho = rho * rho % cp.r
    return rho * rho % cp.r, rho


def dft(x, root, p, force_sum=False):
    """X[k] = sum_i x[i] root^(ik)"""
    m = len(x)
    if m <= DFT_SUM_LIMIT or force_sum:
        return [sum(x[i] * pow(root, i * k, p) for i in range(m)) % p for k in range(m)]
    dom = pm.Domain.__new__(pm.Domain)
    dom.p = p
    return dom._ntt(list(x), root)


def idft(x, root, p, force_sum=False):
    m_inv = pow(len(x), p - 2, p)
    return [v * m_inv % p for v in dft(x, pow(root, p - 2, p), p, force_sum)]


def rows_abc(cp, cs, z):
    """steps 1 and 2"""
    p = cp.r
    nc, ni = cs.num_constraints, cs.num_inputs
    n = 1
    while n < nc + ni:
        n <<= 1
    a, b = [0] * n, [0] * n
    for i in range(nc):
        a[i] = pm.evaluate_constraint(cs.a[i], z, p)
        b[i] = pm.evaluate_constraint(cs.b[i], z, p)
    for j in range(ni):
        a[nc + j] = z[j] % p
    return a, b, [x * y % p for x, y in zip(a, b)]


def witness_map(cp, cs, z):
    p = cp.r
    a, b, c = rows_abc(cp, cs, z)
    n = len(a)
    w, rho = roots(cp, n)

    def shift(v):
        coeffs = idft(v, w, p)
        return dft([x * pow(rho, i, p) % p for i, x in enumerate(coeffs)], w, p)

    a, b, c = shift(a), shift(b), shift(c)
    return [(x * y - u) % p for x, y, u in zip(a, b, c)]


def h_query_scalars(cp, n, t, delta_inv, force_sum=False):
    p = cp.r
    _, rho = roots(cp, n)
    v, acc = [], delta_inv % p
    for _ in range(2 * n - 1):
        v.append(acc)
        acc = acc * t % p
    v.append(0)
    return idft(v, rho, p, force_sum)[1::2]


def abc_at(cp, cs, z, t):
    """(A B - C)(t) for the polynomials of degree < n through the rows a, b, c = a b of steps 1 and 2"""
    p = cp.r
    a, b, c = rows_abc(cp, cs, z)
    lag = pm.Domain(cp, len(a)).lagrange_at(t)
    ev = lambda v: sum(x * l for x, l in zip(v, lag)) % p  # noqa: E731
    return (ev(a) * ev(b) - ev(c)) % p
