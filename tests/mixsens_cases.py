"""Cases and expected values for the rate-mixture gradient tests (test infrastructure; may use oracle/).

Everything expected here comes from the oracle as it stands, on one-category models: with a numeric rate divisor the
normalised matrix does not depend on the mixture, so the model with rate_mixture {rates: [r_c], prior: [1]} IS category c
of the mixture.  site_ll(precise=2) gives ll_{s,c}, site_deriv(precise=2) its edge derivatives; sums run in long double.
    L_{s,c} / L_s                 = exp(ll_{s,c} - ll_s)                                  (log differences: no underflow)
    (dL_{s,c}/dr_c) / L_{s,c}     = sum_e (t_e / r_c) site_deriv_e                         (r_c > 0)
    dL_{s,c}/dr_c at r_c = 0      = 4-point forward difference of exp(ll_{s,c}(r) - ll_s)  (steps h and h / 2, zero_rate_term)
"""
import ctypes

import numpy as np

from phyly_amd import engine as _E, synth

LD = np.longdouble
MIX_KEYS = ("rate_mixture", "gamma_rate_mixture", "normalized_median_gamma_rate_mixture")
FD_H = 1e-3          # first step tried by the forward difference at r = 0 (zero_rate_term)


# ---------------------------------------------------------------- model_and_data documents
def _doc(edges, rates, Q, defs, codes, mixture, divisor, root, dense):
    md = {"edges": edges, "edge_rate_coefficients": [float(v) for v in rates], "rate_matrix": np.asarray(Q).tolist(),
          "rate_divisor": divisor, "root_prior": root}
    if mixture is not None:
        md.update(mixture)
    if dense:
        md["probability_array"] = np.asarray(defs)[np.asarray(codes)].tolist()
    else:
        md["character_definitions"] = np.asarray(defs).tolist()
        md["character_data"] = np.asarray(codes).tolist()
    return md


FIVE_TAXON_EDGES = [[0, 1], [0, 2], [0, 3], [1, 4], [1, 5], [2, 6], [2, 7]]
FOUR_CATEGORIES = {"rate_mixture": {"rates": [0.0, 0.5, 1.3, 2.5], "prior": [0.2, 0.5, 0.0, 0.3]}}   # a rate 0, a prior 0
ONE_CATEGORY = {"rate_mixture": {"rates": [0.8], "prior": [1.0]}}


def five_taxon_doc(S, C, seed, dense=False, mixture=None, divisor=1.3, k=4):
    """5 taxa (3 4 5 6 7): the root has three children, node 2 carries data, edge 1 -> 5 has rate 0, one ambiguity code.
    C = 1: one category of rate 0.8; C = 4: FOUR_CATEGORIES; C = 5: Gamma4 + I; or the mixture given."""
    from helpers import nonreversible_rates
    rng = np.random.default_rng(seed)
    N = 8
    leaves = [3, 4, 5, 6, 7]
    defs = np.vstack([np.eye(k), np.ones((1, k)), rng.choice([0.25, 0.5, 1.0], size=(1, k))])
    codes = np.full((S, N), k, dtype=int)
    base = rng.integers(0, k, (S, 1))                                  # correlated leaves: constant sites occur
    codes[:, leaves] = np.where(rng.random((S, 5)) < 0.6, base, rng.integers(0, k, (S, 5)))
    codes[:, 2] = np.where(rng.random(S) < 0.5, rng.integers(0, k, S), k)
    sub = codes[:, [3, 6, 7]]
    sub[rng.random(sub.shape) < 0.08] = k + 1
    codes[:, [3, 6, 7]] = sub
    rates = rng.uniform(0.05, 0.6, 7)
    rates[4] = 0.0                                                     # edge 1 -> 5
    if mixture is None:
        mixture = {1: ONE_CATEGORY, 4: FOUR_CATEGORIES,
                   5: {"gamma_rate_mixture": dict(gamma_shape=0.7, gamma_categories=4, invariable_prior=0.15)}}[C]
    return _doc(FIVE_TAXON_EDGES, rates, nonreversible_rates(k, rng), defs, codes, mixture, divisor, "equilibrium_distribution", dense)


def caterpillar_doc(T, S, seed, k=4, C=4, leaf_scale=1.0):
    """T-taxon caterpillar, gamma mixture of C categories (C = 2: custom).  leaf_scale < 1 scales the observation rows:
    40 leaves at 1e-8 put every site likelihood below 1e-300, which only a rescaling pass survives."""
    from helpers import nonreversible_rates
    rng = np.random.default_rng(seed)
    edges, nxt, top, leaves = [], 1, 0, []
    for _ in range(T - 1):
        a, b = nxt, nxt + 1
        nxt += 2
        edges += [[top, a], [top, b]]
        leaves.append(a)
        top = b
    leaves.append(top)
    N = nxt
    defs = np.vstack([np.eye(k) * leaf_scale, np.ones((1, k))])
    codes = np.full((S, N), k, dtype=int)
    base = rng.integers(0, k, (S, 1))
    codes[:, leaves] = np.where(rng.random((S, T)) < 0.5, base, rng.integers(0, k, (S, T)))
    mixture = {"gamma_rate_mixture": dict(gamma_shape=0.6, gamma_categories=C)} if C != 2 else \
              {"rate_mixture": {"rates": [0.4, 1.9], "prior": [0.6, 0.4]}}
    Q = nonreversible_rates(k, rng)
    # a numeric divisor near the mean exit rate: edge rates stay expected substitutions per site whatever k is (with a
    # fixed number the 61-state chain would be saturated on every edge and every derivative a cancellation residue)
    return _doc(edges, rng.uniform(0.05, 0.4, len(edges)), Q, defs, codes, mixture, float(1.1 * np.sum(Q) / k),
                "equilibrium_distribution", False)


# ---------------------------------------------------------------- engine set-up through the product's own K0
def product_k0(m):
    """arbplf_k0_prepare of the product for an oracle Model (any mixture form)"""
    lib = _E.load_library()
    mix = synth._K0Mixture()
    mix.mode = {0: 1, 1: 2, 2: 3, 3: 4, 4: 5}[m.mix_mode]
    mix.n = int(m.mix_n)
    keep = []
    if m.mix_rates is not None:
        r = np.ascontiguousarray(m.mix_rates, dtype=np.float64)
        p = np.ascontiguousarray(m.mix_prior, dtype=np.float64)
        keep = [r, p]
        dp = ctypes.POINTER(ctypes.c_double)
        mix.rates, mix.prior = r.ctypes.data_as(dp), p.ctypes.data_as(dp)
    mix.gamma_shape, mix.invariable_prior = float(m.gamma_shape), float(m.pinv)
    lib.arbplf_k0_category_count.argtypes = [ctypes.POINTER(synth._K0Mixture)]
    C = lib.arbplf_k0_category_count(ctypes.byref(mix))
    k = m.k
    Q = np.ascontiguousarray(m.rate_matrix, dtype=np.float64)
    rates, prior, pi, Qn, Qn_lo = np.zeros(C), np.zeros(C), np.zeros(k), np.zeros((k, k)), np.zeros((k, k))
    dp = ctypes.POINTER(ctypes.c_double)
    lib.arbplf_k0_prepare.argtypes = [ctypes.c_int, dp, ctypes.c_int, ctypes.c_double, ctypes.c_int,
                                      ctypes.POINTER(synth._K0Mixture), dp, dp, dp, dp, dp]
    rc = lib.arbplf_k0_prepare(k, Q.ctypes.data_as(dp), int(m.use_eq_divisor), float(m.divisor), int(m.root_mode == 4 or bool(m.use_eq_divisor)),
                               ctypes.byref(mix), *(a.ctypes.data_as(dp) for a in (rates, prior, pi, Qn, Qn_lo)))
    assert rc == C and keep is not None
    return dict(C=C, cat_rates=rates, cat_prior=prior, pi=pi, Qn=Qn, Qn_lo=Qn_lo)


def setup_engine(eng, oracle, md, S=None):
    """tree, model and patterns of a document on an Engine -> (m, w) of the oracle; S: the first S sites only"""
    m = oracle.parse_model(md)
    w = oracle.prepare(m)
    k0 = product_k0(m)
    rw = k0["pi"] if m.root_mode == 4 else (np.asarray(m.root_custom, dtype=float) if m.root_mode == 2 else None)
    eng.set_tree(m.indptr, m.indices, m.preorder)
    eng.set_model(k0["Qn"], m.edge_rates_csr, k0["cat_rates"], k0["cat_prior"], m.root_mode, rw, Qn_lo=k0["Qn_lo"])
    if "probability_array" in md:
        eng.set_patterns_dense(np.ascontiguousarray(np.transpose(m.B[:S], (1, 2, 0))))
    else:
        eng.set_patterns_codes(np.ascontiguousarray(np.asarray(md["character_data"][:S], dtype=np.uint8).T),
                               np.asarray(md["character_definitions"], dtype=float))
    return m, w


# ---------------------------------------------------------------- oracle expectations
def one_category(md, r):
    md1 = {key: v for key, v in md.items() if key not in MIX_KEYS}
    md1["rate_mixture"] = {"rates": [float(r)], "prior": [1.0]}
    return md1


def _model(oracle, md, cache=None, key=None):
    """(m, w) of a document; prepared once per cache and key (the binary128 exponentials of a large k take seconds)"""
    if cache is not None and ("model", key) in cache:
        return cache["model", key]
    m = oracle.parse_model(md)
    mw = (m, oracle.prepare(m))
    if cache is not None:
        cache["model", key] = mw
    return mw


def _site_ll(oracle, md, cache=None, key=None, keep_model=True):
    """keep_model = False: the prepared model is not kept (the difference steps of zero_rate_term, which nothing reuses)"""
    if cache is not None and key in cache:
        return cache[key]
    m, w = _model(oracle, md, cache if keep_model else None, key)
    ll, _ = oracle.site_ll(m, w, B=m.B, precise=2)
    ll = np.asarray(ll, dtype=LD)
    if cache is not None:
        cache[key] = ll
    return ll


def _fd4(f0, f1, f2, f3, h):
    return (-11 * f0 + 18 * f1 - 9 * f2 + 2 * f3) / (6 * LD(h))


def zero_rate_term(oracle, md, ll_s, wt_p, h0=FD_H, cache=None):
    """sum_s wt_p[s] d/dr exp(ll_{s,c}(r) - ll_s) at r = 0 by one-sided 4-point differences at steps h and h / 2
    -> (value at h / 2, |value at h / 2 - value at h|, h).  Truncation falls as h^3 and the rounding of the oracle's
    double ll output rises as 1 / h, so the disagreement of the two steps has a minimum over h: starting at h0, h is
    divided by 4 while the disagreement shrinks, and the step of the smallest disagreement is taken."""
    def g(r):
        with np.errstate(over="ignore"):
            return np.sum(wt_p * np.where(wt_p != 0, np.exp(_site_ll(oracle, one_category(md, r), cache, ("ll", float(r)), keep_model=False) - ll_s), 0))
    g0 = g(0.0)
    best = None
    h = h0
    for _ in range(8):
        fine, coarse = _fd4(g0, g(h / 2), g(h), g(3 * h / 2), h / 2), _fd4(g0, g(h), g(2 * h), g(3 * h), h)
        gap = abs(fine - coarse)
        if best is not None and gap >= best[1]:
            break
        best = (fine, gap, h)
        h /= 4
    return best


def expectations(oracle, md, weights, cache=None):
    """(prior_out [C], rate_out [C], rate_tol [C]) of plk_mixture_sens from the oracle alone, in long double.
    cache: a dict the caller keeps for ONE document; the prepared models and the per-site oracle values, which do not
    depend on the weights, are kept there, so that a second weight vector costs no oracle call.
    rate_tol[c] is the accuracy of the expected rate_out[c] relative to max_c |rate_out|: 0 where the value comes from
    binary128 derivatives, and for a category of rate 0 the larger of 1e-9 and ten times the disagreement of the two
    difference steps (asserted below 1e-8, so that a test cannot hide behind it)."""
    assert not isinstance(md.get("rate_divisor"), str), "the one-category models need a numeric divisor"
    m, w = _model(oracle, md, cache, "mixture")
    C = int(w["C"])
    wt = np.asarray(weights, dtype=LD)
    ll_s = _site_ll(oracle, md, cache, "mixture")
    assert np.all(np.isfinite(ll_s[np.asarray(weights) != 0]))
    t = np.asarray(m.edge_rates_csr, dtype=LD)
    prior_out, rate_out, fd_gap = np.zeros(C, dtype=LD), np.zeros(C, dtype=LD), np.zeros(C, dtype=LD)
    live = np.asarray(weights) != 0
    for c in range(C):
        r, p = float(w["cat_rates"][c]), LD(w["cat_prior"][c])
        md1 = one_category(md, r)
        ll_c = _site_ll(oracle, md1, cache, ("ll", r))
        with np.errstate(over="ignore"):
            ratio = np.where(live, np.exp(ll_c - ll_s), 0)
        prior_out[c] = np.sum(wt * ratio)
        if r > 0:
            if cache is None or ("deriv", r) not in cache:
                m1, w1 = _model(oracle, md1, cache, ("ll", r))
                d = np.asarray(oracle.site_deriv(m1, w1, m1.B, precise=2), dtype=LD)
                if cache is not None:
                    cache["deriv", r] = d
            else:
                d = cache["deriv", r]
            per_site = np.where(live, ratio * (d @ (t / LD(r))), 0)
            rate_out[c] = p * np.sum(wt * per_site)
        else:
            rate_out[c], fd_gap[c], _ = zero_rate_term(oracle, md, ll_s, wt * p, cache=cache)
    scale = np.max(np.abs(rate_out))
    gap = fd_gap / scale if scale > 0 else fd_gap
    assert np.all(gap < 1e-8), "forward difference at r = 0: steps h and h/2 disagree by %s of max|rate_out|" % gap
    tol = np.where(np.asarray(w["cat_rates"]) == 0, np.maximum(LD(1e-9), 10 * gap), 0)
    return prior_out, rate_out, tol


# ---------------------------------------------------------------- the chain rule
def closed_form_chain(rates, prior, exit_rate, prior_out, rate_out):
    """d/drates, d/dprior of a custom mixture by the issue's closed form, in long double (prior None: uniform)"""
    r = np.asarray(rates, dtype=LD)
    n = len(r)
    p = np.asarray(prior, dtype=LD) if prior is not None else np.full(n, LD(1) / n)
    ro, po = np.asarray(rate_out, dtype=LD), np.asarray(prior_out, dtype=LD)
    if not exit_rate:
        return ro, po
    T, expect = np.sum(r * ro), np.sum(r * p)
    return ro - p * T / expect, po - r * T / expect


def dd(x):
    x = np.asarray(x, dtype=LD)
    hi = x.astype(np.float64)
    return np.ascontiguousarray(np.stack([hi, (x - hi.astype(LD)).astype(np.float64)], axis=-1))


def product_chain(mode, n, rates, prior, shape, pinv, exit_rate, prior_out, rate_out):
    """plk_mixture_chain through ctypes -> dict(rc, drates, dprior, dshape, dinv, has_inv, msg); mode as in host_k0.h"""
    lib = _E.load_library()
    vp = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None
    r = np.ascontiguousarray(rates, dtype=np.float64) if rates is not None else None
    p = np.ascontiguousarray(prior, dtype=np.float64) if prior is not None else None
    po, ro = dd(prior_out), dd(rate_out)
    dr, dpv = np.full(max(n, 1), np.nan), np.full(max(n, 1), np.nan)
    ds, di = np.full(1, np.nan), np.full(1, np.nan)
    has = ctypes.c_int(-1)
    err = ctypes.create_string_buffer(200)
    lib.plk_mixture_chain.restype = ctypes.c_int
    rc = lib.plk_mixture_chain(int(mode), int(n), vp(r), vp(p), float(shape), float(pinv), 1 if exit_rate else 0, vp(po), vp(ro),
                               vp(dr), vp(dpv), vp(ds), vp(di), ctypes.byref(has), err, 200)
    return dict(rc=rc, drates=dr, dprior=dpv, dshape=ds[0], dinv=di[0], has_inv=has.value, msg=err.value.decode())
