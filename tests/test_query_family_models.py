"""CPU only: the models of tests/test_gpu_query_variants.py can tell a wrong kernel from a right one.

For each of them the oracle alone shows that a plausible bug of the posterior, pair-sum or mixture-gradient kernels moves
the values those tests compare (posteriors and site log likelihoods; W; prior_out and rate_out) by far more than their
bars (1e-12 and tighter): the root prior replaced by the equilibrium distribution, the data on internal nodes dropped,
W[c][e] transposed, two categories exchanged, the rate-0 edge given a positive rate, and, for the pair sums, two children
of a multifurcation exchanged."""

import numpy as np
import pytest

import catpost_cases
import mixsens_cases
import qgrad_cases
from helpers import K4_MODELS, QUERY_MODEL, family_workload, numeric_divisor_doc, query_workload

TEETH = 1e-6        # a bug must move a checked quantity by this much of its scale: six decades over the 1e-12 bars
MODELS = K4_MODELS + (QUERY_MODEL,)
FAMILY_KS = (2, 5, 13, 27, 48)
LD = np.longdouble


def _values(oracle, md, factored, mix=True):
    """what tests/test_gpu_query_variants.py compares, from the oracle, unit weights"""
    m = oracle.parse_model(md)
    w = oracle.prepare(m)
    post, rate, sll = catpost_cases.posteriors(oracle, m, w, precise=2, B=m.B)
    if factored:             # k >= 27: the oracle's long-double pass, ten decades finer than TEETH
        W = qgrad_cases.oracle_W_factored(oracle, m, w, np.ones(m.S), precise=1 if m.k >= 27 else 2)
    else:
        W = qgrad_cases.oracle_W(oracle, m, w, np.ones(m.S))
    out = dict(post=post, ll=sll, W=W)
    if mix:
        po, ro, _ = mixsens_cases.expectations(oracle, md, np.ones(m.S))
        out["mix"] = np.stack([po, ro])
    return out, m, w


def _moved(a, b):
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def _swap01(x, axis):
    idx = np.arange(x.shape[axis])
    idx[[0, 1]] = [1, 0]
    return np.take(x, idx, axis=axis)


def _check_model(oracle, wl, S, factored, data_nodes):
    """-> {perturbation: smallest ratio moved / scale over the quantities it must move}"""
    codes = wl.simulate(S)
    md = numeric_divisor_doc(wl, codes)
    # k >= 27: the one-category models of the mixture sums cost a binary128 matrix exponential per edge each (3 s per
    # model at k = 48), so there the models are compared on the posteriors, the log likelihoods and W alone
    remix = wl.k < 27
    base, m, w = _values(oracle, md, factored, remix)
    C = int(w["C"])
    seen = {}
    moved = ("ll", "W") + (("mix",) if remix else ()) + (("post",) if C > 1 else ())

    def against(name, other, keys):
        seen[name] = min(_moved(other[key], base[key]) for key in keys)

    # the model as a document: every quantity must move
    if wl.root != "equilibrium":
        # a root that carries data meets its prior as one factor of the site likelihood: only the ll by-product of
        # plk_cat_posterior sees it (family k = 27)
        other, _, _ = _values(oracle, dict(md, root_prior="equilibrium_distribution"), factored, remix)
        against("root prior", other, ("ll",) if int(wl.preorder[0]) in data_nodes else moved)
    if len(data_nodes):
        dropped = codes.copy()
        assert np.any(dropped[data_nodes] != wl.k)
        dropped[data_nodes] = wl.k                      # the all-ones row
        other, _, _ = _values(oracle, numeric_divisor_doc(wl, dropped), factored, remix)
        against("internal data", other, moved)
    zero = [i for i, r in enumerate(md["edge_rate_coefficients"]) if r == 0.0]
    if zero:
        rates = list(md["edge_rate_coefficients"])
        rates[zero[0]] = 0.05
        other, _, _ = _values(oracle, dict(md, edge_rate_coefficients=rates), factored, remix)
        against("rate-0 edge", other, moved)
    # index mistakes, on the values themselves
    against("W transposed", dict(W=base["W"].transpose(0, 1, 3, 2)), ("W",))
    if C > 1:
        other = dict(post=_swap01(base["post"], 1), W=_swap01(base["W"], 0))
        if remix:
            other["mix"] = _swap01(base["mix"], 1)
        against("categories exchanged", other, tuple(other))
    deg = np.diff(m.indptr)
    if np.max(deg) >= 3:
        a = int(np.argmax(deg >= 3))
        e0 = int(m.indptr[a])
        Wx = base["W"].copy()
        Wx[:, [e0, e0 + 1]] = Wx[:, [e0 + 1, e0]]
        against("children exchanged", dict(W=Wx), ("W",))
    for name, ratio in seen.items():
        assert ratio >= TEETH, (wl.name, name, ratio)
    return seen


@pytest.mark.parametrize("model", MODELS)
def test_k4_query_model_detects_plausible_kernel_bugs(oracle, model):
    """8 simulated sites.  Smallest ratio observed over the five models: 3.0e-4 (wide, the rate-0 edge given rate 0.05);
    then 8.0e-4 (balanced32, the root prior) and 9.4e-4 (wide, two children of node 13 exchanged: two of its edges have
    rates 0.11 and 0.07); W transposed moves W by all of max|W|, two categories exchanged by 0.19 at the least"""
    wl = query_workload(model)
    seen = _check_model(oracle, wl, 8, False, list(getattr(wl, "data_nodes", ())))
    want = {"W transposed"}
    if model != "wide":
        want.add("root prior")
    if model in ("irregular", "wide"):
        want |= {"internal data", "rate-0 edge", "children exchanged"}
    if model != "balanced32":
        want.add("categories exchanged")
    assert set(seen) == want
    print(model, {n: "%.2g" % v for n, v in seen.items()})


@pytest.mark.parametrize("k", FAMILY_KS)
def test_family_query_model_detects_plausible_kernel_bugs(oracle, k):
    """the models of the generic instantiations, 4 simulated sites, W from oracle_W_factored.  Smallest ratio observed:
    2.0e-5 (k = 48, the root prior), then 1.2e-4 (k = 5, two categories exchanged)"""
    wl = family_workload(k)
    leaf = wl.indptr[1:] == wl.indptr[:-1]
    inner = list(np.flatnonzero(~leaf)[::3]) if wl.internal_data else []
    seen = _check_model(oracle, wl, 4, True, inner)
    want = {"W transposed", "categories exchanged", "root prior"}
    if wl.internal_data:
        want.add("internal data")
    assert set(seen) == want
    print(k, {n: "%.2g" % v for n, v in seen.items()})
