"""CPU: the reference of tests/test_gpu_k1_extremes.py earns its bar before the kernel is held to it.

tests/test_gpu_k1_extremes.py compares the device's transition matrices with the oracle's entry by entry, to 2 ulp, on a
ladder of edge rates from 0 to the documented limit of K1 (r_c t_e |Qn|_inf just under 2^40) and with the category rates
0, 1e-3, 1 and 50 (tests/k1_cases.py).  That bar takes the oracle's rounded-double P for a correct rounding.  Here the
oracle is held, on the same ladder and mixture, to
  * closed forms evaluated by mpmath at 400 bits: the k-state equal-rates model (k = 4, 13), the general two-state
    model, and the pure-birth chain with an absorbing last state, whose entries m steps above the diagonal are the
    Poisson terms e^(-x) x^m / m! (the multi-step entries, down to 3.8e-280; at the long rungs they are below 1e-1700
    and the double is exactly 0) and whose lower triangle is exactly 0;
  * mpmath's own matrix exponential at 400 bits on the non-reversible k = 4 model of the GPU test, from the double-double
    Qn the engine is given.
The bar is 0.5 + 2^-6 ulp of the exact value: a correct rounding, plus what binary128 keeps after 45 squarings at k <= 64
(113 - 45 - 6 = 62 bits, 2^-9 ulp of a double) with margin.  Measured: see DESIGN.md section 2.

Teeth: the same ladder tells a dropped low word of Qn (more than 1e-10 relative on some entry), and the single-entry
sites tell a transposed P and the category rate of the neighbouring category (more than 1e-6 in some site's ll)."""
import math

import numpy as np
import pytest

import k1_cases as K
from helpers import oracle_model

import mpmath as mp

mp.mp.prec = 400

HALF_ULP = 0.5 + 2.0 ** -6


def _json_star(Q, divisor, rates, mixed=True):
    k = len(Q)
    md = dict(edges=K.STAR, edge_rate_coefficients=[float(r) for r in rates], rate_matrix=np.asarray(Q, dtype=float).tolist(),
              rate_divisor=divisor, character_definitions=np.eye(k).tolist() + [[1.0] * k],
              character_data=[[k] * 13])
    if mixed:
        md["rate_mixture"] = dict(rates=K.MIX["rates"], prior=K.MIX["prior"])
    return md


def _oracle_P(oracle, Q, divisor):
    """-> (P [4][12][k][k] of the oracle, the 12 edge rates): the ladder with its top rung at the limit for this Qn"""
    Qn = np.asarray(Q, dtype=float) / divisor
    np.fill_diagonal(Qn, 0.0)
    top = K.LIMIT * (1.0 - 2.0 ** -20) / (max(K.MIX["rates"]) * float(np.max(Qn.sum(axis=1)) * 2))     # |Qn|_inf = 2 x exit rate
    rates = [top if r is None else r for r in K.LADDER]
    m = oracle.parse_model(_json_star(Q, divisor, rates))
    w = oracle.prepare(m)
    assert w["P"].shape == (4, 12, len(Q), len(Q))
    return w["P"], rates


def _worst(P, exact, floor=K.SMALLEST):
    """largest distance in ulp of the exact value and the smallest non-zero exact entry; exact zeros must be zeros"""
    worst, smallest = 0.0, math.inf
    for idx in np.ndindex(P.shape):
        x = exact(*idx)
        if x == 0:
            assert P[idx] == 0.0, idx
            continue
        if P[idx] == 0.0:
            assert x < mp.mpf(K.UNDERFLOWN), (idx, mp.nstr(x, 5))      # far beneath the subnormals: the double is exactly 0, nothing else
            continue
        xd = float(x)
        assert abs(xd) >= floor, (idx, xd)
        worst = max(worst, float(abs(mp.mpf(float(P[idx])) - x) / mp.mpf(float(np.spacing(abs(xd))))))
        smallest = min(smallest, abs(xd))
    return worst, smallest


def _scale(c, e, rates):
    return mp.mpf(K.MIX["rates"][c]) * mp.mpf(rates[e])


@pytest.mark.parametrize("k", [4, 13])
def test_equal_rates_closed_form(oracle, k):
    """P_ij = (1 - e^(-k mu s)) / k off the diagonal, through expm1"""
    mu, divisor = 0.7, 1.6
    P, rates = _oracle_P(oracle, np.full((k, k), mu), divisor)
    rate = mp.mpf(mu) / mp.mpf(divisor)

    def exact(c, e, i, j):
        off = -mp.expm1(-k * rate * _scale(c, e, rates)) / k
        return off if i != j else 1 - (k - 1) * off
    worst, smallest = _worst(P, exact)
    print("equal rates k=%d: worst %.3f ulp, smallest entry %.3g" % (k, worst, smallest))
    assert worst <= HALF_ULP


def test_two_state_closed_form(oracle):
    a, b, divisor = 3.1, 0.4, 0.9
    P, rates = _oracle_P(oracle, [[0, a], [b, 0]], divisor)
    an, bn = mp.mpf(a) / mp.mpf(divisor), mp.mpf(b) / mp.mpf(divisor)

    def exact(c, e, i, j):
        s = _scale(c, e, rates)
        gone = -mp.expm1(-(an + bn) * s)                    # 1 - e^(-(a + b) s)
        off = (an if i == 0 else bn) * gone / (an + bn)
        return off if i != j else 1 - off
    worst, smallest = _worst(P, exact)
    print("two states: worst %.3f ulp, smallest entry %.3g" % (worst, smallest))
    assert worst <= HALF_ULP


def test_birth_chain_closed_form(oracle):
    """Poisson entries above the diagonal, the absorbing column their complement, exact zeros below the diagonal"""
    k = K.BIRTH_K
    Q = np.zeros((k, k))
    Q[np.arange(k - 1), np.arange(1, k)] = K.BIRTH_LAMBDA
    P, rates = _oracle_P(oracle, Q, K.BIRTH_DIVISOR)
    lam = mp.mpf(K.BIRTH_LAMBDA) / mp.mpf(K.BIRTH_DIVISOR)

    def exact(c, e, i, j):
        if j < i:
            return mp.mpf(0)
        x = lam * _scale(c, e, rates)
        if i == k - 1:
            return mp.mpf(1)
        if x == 0:
            return mp.mpf(1 if i == j else 0)
        if j < k - 1:
            return mp.exp(-x) * x ** (j - i) / mp.factorial(j - i)
        return mp.gammainc(k - 1 - i, 0, x, regularized=True)          # sum of the Poisson terms from k - 1 - i on
    assert max(rates) > 1e6 and 0.999 * K.LIMIT < max(K.MIX["rates"]) * max(rates) * 2 * float(lam) < K.LIMIT      # the whole ladder
    worst, smallest = _worst(P, exact, K.BIRTH_SMALLEST)
    print("birth chain: worst %.3f ulp, smallest entry %.3g" % (worst, smallest))
    assert smallest < 1e-270           # the seven-step entry on the shortest rung under the slowest category
    assert worst <= HALF_ULP


@pytest.fixture(scope="module")
def k4(oracle):
    """the k = 4 model of the GPU test with the mixture: workload, oracle model and workspace, mpmath's exponentials
    from the double-double Qn (with its low word, and without)"""
    wl = K.star_workload(4, True)
    m, w = oracle_model(oracle, wl, K.entry_sites(4, [(0, 0, 0)]))
    k0 = wl.prepare()
    assert np.array_equal(k0["cat_rates"], K.MIX["rates"])
    hi, lo = mp.matrix(k0["Qn"].tolist()), mp.matrix(k0["Qn_lo"].tolist())
    full, dropped = {}, {}
    # mpmath's series stops at an absolute bound of one unit of the working precision: 1400 bits put it at 1e-421, sixteen
    # digits and more below the three-step entry on the shortest rung (7e-135)
    with mp.workprec(1400):
        for c in range(4):
            for e in range(12):
                s = mp.mpf(float(k0["cat_rates"][c])) * mp.mpf(float(wl.edge_rates_csr[e]))
                full[c, e], dropped[c, e] = mp.expm((hi + lo) * s), mp.expm(hi * s)
    return wl, m, w, full, dropped


def test_nonreversible_k4_against_mpmath(k4):
    wl, m, w, full, _ = k4
    assert 0.999 * K.LIMIT < np.max(wl.prepare()["cat_rates"]) * np.max(wl.edge_rates_csr) * K.qnorm(wl.prepare()["Qn"]) < K.LIMIT
    worst, smallest = _worst(w["P"], lambda c, e, i, j: full[c, e][i, j] if wl.edge_rates_csr[e] * K.MIX["rates"][c] else mp.mpf(int(i == j)))
    print("non-reversible k=4: worst %.3f ulp, smallest entry %.3g" % (worst, smallest))
    assert worst <= HALF_ULP


def test_ladder_tells_a_dropped_low_word_of_Qn(k4):
    wl, m, w, full, dropped = k4
    worst = max(float(abs(dropped[ce][i, j] - full[ce][i, j]) / full[ce][i, j]) for ce in full for i in range(4) for j in range(4)
                if full[ce][i, j] != 0)
    benign = max(float(abs(dropped[c, e][i, j] - full[c, e][i, j]) / full[c, e][i, j]) for c in range(4) for e in range(12)
                 for i in range(4) for j in range(4) if 0 < wl.edge_rates_csr[e] * K.MIX["rates"][c] <= 0.3)
    print("dropped low word of Qn: %.3g relative on the ladder, %.3g at products up to 0.3" % (worst, benign))
    assert worst > 1e-10
    assert benign < 1e-15              # what the benign lengths of the older tests could see: nothing


def test_sites_tell_a_transposed_P_and_a_neighbouring_category(oracle, k4):
    wl, m, w, _, _ = k4
    codes = K.entry_sites(4, K.all_entries(w["P"][2]))                 # non-zero under the rate-1 category
    ll = lambda ws: oracle.site_ll(m, ws, codes=np.ascontiguousarray(codes.T), defs=wl.defs, precise=1)[0]
    want = ll(w)
    assert np.all(np.isfinite(want))
    transposed = dict(w, P=np.ascontiguousarray(np.swapaxes(w["P"], -1, -2)))
    neighbour = dict(w, P=np.ascontiguousarray(np.roll(w["P"], 1, axis=0)))      # every category reads its neighbour's matrices
    for name, other in (("transposed", transposed), ("neighbouring category", neighbour)):
        moved = np.max(np.abs(ll(other) - want))
        print("%s: some site's ll moves by %.3g" % (name, moved))
        assert moved > 1e-6, name


@pytest.mark.parametrize("k", [4, 13, 27, 61, "birth"])
def test_no_subnormal_enters_a_comparison(oracle, k):
    """every non-zero reference entry of the GPU test's matrices is above 1e-250 (k = 61: the 12 x 4 matrices of the
    mixture model only; the birth chain: all but two, see k1_cases); zeros are where they must be: the rate-0 edge, the rate-0 category, below the birth chain's diagonal"""
    wl = K.star_workload(k, True)
    kk = wl.k
    m, w = oracle_model(oracle, wl, K.entry_sites(kk, [(0, 0, 0)]))
    P = w["P"]
    nz = P[P != 0]
    print("k=%s: smallest non-zero reference entry %.3g, %d exact zeros" % (k, nz.min(), np.sum(P == 0)))
    if k == "birth":                   # k1_cases: the seven-step entry on the shortest rung under the categories 1e-3 and 1
        assert nz.min() >= K.BIRTH_SMALLEST and np.sum(nz < K.SMALLEST) == 2 and P[1, 1, 0, 7] < P[2, 1, 0, 7] < K.SMALLEST
    else:
        assert nz.min() >= K.SMALLEST
    eye = np.broadcast_to(np.eye(kk), (12, kk, kk))
    assert np.array_equal(P[0], eye) and np.array_equal(P[:, 0], np.broadcast_to(np.eye(kk), (4, kk, kk)))
    live = P[1:, 1:]
    if k == "birth":
        assert np.all(live[..., np.tril_indices(kk, -1)[0], np.tril_indices(kk, -1)[1]] == 0)
        assert np.all(live[..., :, kk - 1] > 0)               # the absorbing column; Poisson entries may have underflown to 0
    else:
        assert np.all(live > 0)
    np.testing.assert_allclose(P.sum(axis=-1), 1.0, rtol=0, atol=1e-14)
