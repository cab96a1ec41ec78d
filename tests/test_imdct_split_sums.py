"""The long-block IMDCT of k_dec_stream: its stages' nine-term sums as four-term sums over the sums and differences of the pairs
(k, 8 - k) plus a centre term (csrc/k_decode_stream.hpp; signs, derivation and error bound in csrc/mp3s_tables.cpp).  No GPU: the
algebra on the library's own tables, and the kernel's fp64 operation order restated in numpy against the bound the derivation states."""
from fractions import Fraction

import numpy as np
import pytest

LD = np.longdouble
U = 2.0 ** -53
# what the derivation in mp3s_tables.cpp states for the split sums: |y_fast - y_true| <= ((g4 + 3u) sqrt2 + 6.02 u) B < 16 u B
BOUND_U = 16.0

pytestmark = pytest.mark.skipif(np.finfo(LD).nmant < 63, reason="needs an 80-bit long double for the true sums")


@pytest.fixture(scope="module")
def tabs(mlib):
    t = mlib.debug_tables()
    return np.array(t["imdct_rot"], dtype=np.float64)[0].copy(), np.array(t["imdct_pq"], dtype=np.float64).copy()


def adversarial():
    """The inputs the sums' symmetry could go wrong on: all 18 lines equal, alternating signs, one line only, v[k] = -v[17-k]."""
    out = [np.ones(18), -np.ones(18), np.array([(-1.0) ** k for k in range(18)]), np.array([(-1.0) ** (k // 2) for k in range(18)])]
    for k in range(18):
        e = np.zeros(18)
        e[k] = 1.0 + k / 7.0
        out.append(e)
    half = np.array([0.3, -1.7, 2.9, 1e-3, 5.5, -0.25, 7.0, 1.0 / 3.0, -2.0])
    out.append(np.concatenate([half, -half[::-1]]))         # v[k] = -v[17-k]
    out.append(np.concatenate([half, half[::-1]]))          # ... and its even twin
    return out


def y_true(v):
    """y[n] = sum_k v[k] cos((2n+1)(2k+1) pi/72) in long double; the multiple of pi/72 reduced modulo its period in integers first."""
    pil = LD("3.14159265358979323846264338327950288")
    n, k = np.arange(18)[:, None], np.arange(18)[None, :]
    c = np.cos((((2 * n + 1) * (2 * k + 1)) % 144).astype(LD) * pil / LD(72))
    return np.asarray(v, dtype=LD) @ c.T


def centre(m):
    """(sign of p[4] in P[m], sign of q[4] in Q[m]): cos(m pi/2), sin(m pi/2)."""
    return ((-1) ** (m // 2), 0) if m % 2 == 0 else (0, (-1) ** ((m - 1) // 2))


def stages_exact(p, q, pq, split):
    """y from (p, q) by the ten stages in exact rationals: the nine-term sums, or the kernel's split form of them."""
    y = [Fraction(0)] * 18
    for m in range(10):
        cs, sn = [Fraction(x) for x in pq[m, :9]], [Fraction(x) for x in pq[m, 9:]]
        if not split:
            P, Q = sum(a * b for a, b in zip(p, cs)), sum(a * b for a, b in zip(q, sn))
        else:
            sp, sq = centre(m)
            P, Q = sp * p[4], sq * q[4]
            for k in range(4):
                if m % 2 == 0:
                    P += (p[k] + p[8 - k]) * cs[k]
                    Q += (q[k] - q[8 - k]) * sn[k]
                else:
                    P += (p[k] - p[8 - k]) * cs[k]
                    Q += (q[k] + q[8 - k]) * sn[k]
            if m == 9:
                P = Fraction(0)
            if m == 0:
                Q = Fraction(0)
        if m <= 8:
            y[2 * m] = P + Q
        if m >= 1:
            y[2 * m - 1] = P - Q
    return y


def test_split_sums_equal_the_nine_term_sums_and_the_transform(tabs):
    """In exact arithmetic on the table's own doubles the two forms differ only by what the table's entries differ from their mirror
    images: entry 8 - k against +-entry k (each within u/2 of the same true value: u per pair) and the centre entry against 0 or +-1
    (long double's rounding of pi/2).  Both lie within the factors' share of the bound from the true transform: u/2 per factor, two
    factors per line in the rotations (u B) and one per term in the stages (u/2 (sum |p| + sum |q|) <= 0.71 u B)."""
    rot, pq = tabs
    rng = np.random.default_rng(5)
    vs = adversarial() + [rng.standard_normal(18) * 10.0 ** rng.integers(-6, 6) for _ in range(40)]
    worst_forms, worst_true = 0.0, 0.0
    for v in vs:
        x, xm = [Fraction(a) for a in v[:9]], [Fraction(a) for a in v[::-1][:9]]
        c, s = [Fraction(a) for a in rot[0::2]], [Fraction(a) for a in rot[1::2]]
        p = [x[k] * c[k] + xm[k] * s[k] for k in range(9)]
        q = [-x[k] * s[k] + xm[k] * c[k] for k in range(9)]
        direct, split = stages_exact(p, q, pq, False), stages_exact(p, q, pq, True)
        spq = float(sum(abs(a) for a in p) + sum(abs(a) for a in q))
        B = float(np.abs(v).sum())
        d_forms = max(abs(float(a - b)) for a, b in zip(direct, split))
        yt = y_true(v)
        d_true = max(abs(float(LD(float(a)) + LD(float(a - Fraction(float(a)))) - t)) for a, t in zip(split, yt))
        worst_forms, worst_true = max(worst_forms, d_forms / (U * spq)), max(worst_true, d_true / (U * B))
        assert d_forms <= 1.01 * U * spq, (v, d_forms / (U * spq))
        assert d_true <= 1.8 * U * B, (v, d_true / (U * B))
    print("split against nine-term sums: %.3f u (sum |p| + sum |q|); split against the true transform: %.3f u B" % (worst_forms, worst_true))


# ---- the kernel's order in fp64.  numpy has no fused multiply-add: fma(a, b, c) correctly rounded from error-free transformations
#      (a b = ph + pl, ph + c = sh + sl, both exact) and a last step in long double that is checked against the exact residual.
def _two_prod(a, b):
    ph = a * b
    sa, sb = a * 134217729.0, b * 134217729.0
    ah, bh = sa - (sa - a), sb - (sb - b)
    al, bl = a - ah, b - bh
    return ph, ((ah * bh - ph) + ah * bl + al * bh) + al * bl


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def fma(a, b, c):
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    ph, pl = _two_prod(a, b)
    sh, sl = _two_sum(ph, c)
    r = (sh.astype(LD) + (sl.astype(LD) + pl.astype(LD))).astype(np.float64)
    # the residual of r, exact but for a rounding 2^-64 below itself: beyond half a unit in r's last place, r was rounded twice
    e = ((sh - r).astype(LD) + sl.astype(LD)) + pl.astype(LD)
    half = (np.abs(np.nextafter(r, np.inf) - r)).astype(LD) / 2
    half_dn = (np.abs(r - np.nextafter(r, -np.inf))).astype(LD) / 2
    r = np.where(e > half, np.nextafter(r, np.inf), r)
    return np.where(e < -half_dn, np.nextafter(r, -np.inf), r)


def test_the_emulated_fma_is_correctly_rounded():
    rng = np.random.default_rng(9)
    a, b = rng.standard_normal(600), rng.standard_normal(600)
    c = np.concatenate([rng.standard_normal(200), -(a[200:400] * b[200:400]) * (1 + rng.standard_normal(200) * 1e-15),     # cancellation
                        (a[400:] * b[400:]) * 2.0 ** rng.integers(-60, 60, 200)])
    # ties and near-ties of the last rounding: (1 + 2^-52 k) + 2^-53 (1 + tiny)
    a = np.concatenate([a, np.full(8, 2.0 ** -53)])
    b = np.concatenate([b, 1.0 + np.array([0.0, 2.0 ** -30, -2.0 ** -30, 2.0 ** -52, 0.0, 2.0 ** -30, -2.0 ** -30, 2.0 ** -52])])
    c = np.concatenate([c, np.array([1.0, 1.0, 1.0, 1.0, 1.0 + 2.0 ** -52, 1.0 + 2.0 ** -52, 1.0 + 2.0 ** -52, 1.0 + 2.0 ** -52])])
    got = fma(a, b, c)
    for x, y, z, g in zip(a, b, c, got):
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        # correctly rounded: no double is nearer (and of two equally near, the even one: what float(Fraction) gives)
        assert float(exact) == g, (x, y, z, g, float(exact))


def kernel_rows(v, rot, pq):
    """y[0..17] of every row of v (N x 18) in the kernel's operation order (k_dec_stream, long windows)."""
    c, s = rot[0::2], rot[1::2]
    p = [fma(v[:, 17 - k], s[k], v[:, k] * c[k]) for k in range(9)]
    q = [fma(v[:, 17 - k], c[k], -(v[:, k] * s[k])) for k in range(9)]
    ap, dp = [p[k] + p[8 - k] for k in range(4)], [p[k] - p[8 - k] for k in range(4)]
    aq, dq = [q[k] + q[8 - k] for k in range(4)], [q[k] - q[8 - k] for k in range(4)]
    y = np.zeros((v.shape[0], 18))
    for m in range(10):
        sp, sq = centre(m)
        P, Q = sp * p[4] if sp else np.zeros(v.shape[0]), sq * q[4] if sq else np.zeros(v.shape[0])
        for k in range(4):
            if m != 9:
                P = fma(ap[k] if m % 2 == 0 else dp[k], pq[m, k], P)
            if m != 0:
                Q = fma(dq[k] if m % 2 == 0 else aq[k], pq[m, 9 + k], Q)
        if m <= 8:
            y[:, 2 * m] = P + Q
        if m >= 1:
            y[:, 2 * m - 1] = P - Q
    return y


def test_kernel_order_stays_within_the_derived_bound(tabs):
    """10^5 vectors -- random at many scales, sparse, and the adversarial families scaled and perturbed -- through the kernel's order in
    fp64: every output within the derivation's 16 u sum |v| of the true transform.  (The asserted number is the derivation's, and it is
    below the 22 u the guard's constant kappa_dct4 grants this route.)"""
    rot, pq = tabs
    rng = np.random.default_rng(11)
    n = 100000
    v = rng.standard_normal((n, 18)) * 10.0 ** rng.integers(-8, 8, size=(n, 1))
    v[20000:40000] *= rng.random((20000, 18)) < 0.25                                            # a few lines only
    v[40000:50000] = np.sign(v[40000:50000]) * 10.0 ** rng.integers(-3, 4, size=(10000, 1))     # equal magnitudes, random signs
    adv = np.array(adversarial())
    reps = 10000 // len(adv)
    block = np.tile(adv, (reps, 1)) * (1.0 + rng.standard_normal((reps * len(adv), 1)))         # the families, scaled as a whole
    v[50000:50000 + len(block)] = block
    v[60000:60000 + len(block)] = block * (1.0 + rng.standard_normal(block.shape) * 2.0 ** -50)  # ... and off by last places
    v[:len(adv)] = adv
    y = kernel_rows(v, rot, pq)
    B = np.abs(v).sum(axis=1)
    ok = B > 0
    r = np.abs(y.astype(LD) - y_true(v)).max(axis=1)[ok] / (LD(U) * B[ok].astype(LD))
    print("kernel order against the true transform: largest %.3f u B, mean %.3f u B over %d vectors (bound %.0f u B)" % (float(r.max()), float(r.mean()), int(ok.sum()), BOUND_U))
    assert float(r.max()) <= BOUND_U
    assert not y[~ok].any()
