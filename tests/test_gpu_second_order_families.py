"""GPU: plk_second_order / plk_hess beyond k = 4 and under site chunks, against the oracle ("Second
order beyond k = 4").

second_order_generic (k_down_store<K> + k_up<K, true, false> on edge-modified models, K = 2 .. 64) on
helpers.FAMILY_MODELS: non-reversible Q, unequal category priors, a rate-0 category, every root prior, data on internal
nodes; on conserved data (second_order_cases.conserved_codes), which tests/test_second_order_family_models.py shows on
the CPU to tell a wrong pass from a right one.  Also: the dense layout at k = 4, site chunks with a ragged last chunk on
both drivers, rescaled nodes at k = 13, the JSON drivers above k = 8, and two engines.

Every engine case calls plk_second_order and plk_hess and asserts the pass it ran on (PLK_INFO_UPDOWN_KERNEL), H == H^T
and plk_hess == the Hessian of plk_second_order bit for bit, and three bars against the oracle's long-double values
(second_order_cases.Reference, itself held to binary128 on its first sites):
  (a) max|dH| <= 1e-11 max|H|                           the project's bar for Hessians
  (b) max_ij |dH_ij| / (d_i d_j) <= 1e-11               the same number at each edge pair's own scale (edge_scale)
  (c) max|dg| <= 1e-12 sum_s |w_s| max_i |g_s,i|        the gradient, as test_gpu_k4_variants.test_second_order holds it
(a) alone admits an error of 3e-7 of a long edge's own curvature on these trees: entries scale like 1 / (t_i t_j)."""
import json

import numpy as np
import pytest

from helpers import family_workload, k4_workload, oracle_model
import mixsens_cases
import second_order_cases as cases
from test_gpu_hess import _check as _check_table
from test_gpu_k4_variants import _reset, _set_options

pytestmark = pytest.mark.gpu
GENERIC, HESS4 = 2, 5
BAR, GRAD_BAR = 1e-11, 1e-12


@pytest.fixture(scope="module")
def eng():
    from phyly_amd.engine import Engine
    e = Engine(0)
    yield e
    _reset(e)
    e.close()


_REFS = {}


def _family(oracle, k, S):
    """(workload, codes, Reference) of family_workload(k) on conserved_codes(wl, S, S), built once"""
    if (k, S) not in _REFS:
        wl = family_workload(k) if not isinstance(k, str) else k4_workload(k)
        codes = cases.conserved_codes(wl, S, S)
        m, w = oracle_model(oracle, wl, codes)
        _REFS[k, S] = (wl, codes, cases.Reference(oracle, m, w, wl.defs[codes.T]))
    return _REFS[k, S]


def _hold(eng, ref, wts, kernel, label, bar=BAR):
    """both calls under weights wts (None: none), the structural assertions and the three bars"""
    from phyly_amd import engine as E
    eng.set_site_weights(wts)
    try:
        g, H2 = eng.second_order()
        k2 = eng.info(E.INFO_UPDOWN_KERNEL)
        H1 = eng.hess()
        k1 = eng.info(E.INFO_UPDOWN_KERNEL)
    finally:
        eng.set_site_weights(None)
    assert (k2, k1) == (kernel, kernel), label
    assert np.array_equal(H2, H2.T), label
    assert np.array_equal(H1, H2), label
    gw, Hw, d, gscale = ref.sums(wts)
    assert np.all(d > 0), label
    ea = float(np.max(np.abs(H2 - Hw)) / np.max(np.abs(Hw)))
    eb = cases.scaled_err(H2, Hw, d)
    ec = float(np.max(np.abs(g - gw)) / gscale)
    print("second order %s: (a) %.3g (b) %.3g (c) %.3g" % (label, ea, eb, ec))
    assert ea <= bar, (label, "a", ea)
    assert eb <= bar, (label, "b", eb)
    assert ec <= GRAD_BAR, (label, "c", ec)
    return H2


# ------------------------------------------------------------------ the family matrix
@pytest.mark.parametrize("S", cases.FAMILY_SIZES)
@pytest.mark.parametrize("k", cases.FAMILY_KS)
def test_family(eng, oracle, k, S):
    wl, codes, ref = _family(oracle, k, S)
    wl.setup_engine(eng)
    try:
        _set_options(eng, {})
        eng.set_patterns_codes(codes, wl.defs)
        _hold(eng, ref, None, GENERIC, "k=%d S=%d" % (k, S))
        _hold(eng, ref, cases.weights_with_zeros(S, S), GENERIC, "k=%d S=%d weighted" % (k, S))
    finally:
        _reset(eng)


# ------------------------------------------------------------------ the dense layout at k = 4
@pytest.mark.parametrize("model", ["irregular", "balanced32"])
def test_dense_layout_k4(eng, oracle, model):
    """the same observations as compact codes (the k = 4 pass) and as a dense array (pat_mode 2: the generic pass)"""
    S = 65
    wl, codes, ref = _family(oracle, model, S)
    wl.setup_engine(eng)
    wts = cases.weights_with_zeros(S, S)
    try:
        _set_options(eng, {})
        eng.set_patterns_codes(codes, wl.defs)
        _hold(eng, ref, wts, HESS4, model + " codes")
        eng.set_patterns_dense(np.ascontiguousarray(wl.defs[codes].transpose(0, 2, 1)))      # [N][k][S]
        _hold(eng, ref, wts, GENERIC, model + " dense")
        _hold(eng, ref, None, GENERIC, model + " dense unweighted")
    finally:
        _reset(eng)


# ------------------------------------------------------------------ site chunks
# PLK_OPT_SITE_CHUNK is rounded down to whole blocks (64 sites on the generic pass, 256 on the k = 4 pass), so every case
# below ends in a chunk of one site, after 2 (k > 4), 4 (k = 4 forced generic) or 1 (k = 4 pass) full chunks: the chunk
# loop adds into G and Hrow, and reads the weights at h->d_w + s0
CHUNKS = [("irregular", 257, 100, 0, HESS4), ("irregular", 257, 100, 1, GENERIC),
          (13, 129, 64, 0, GENERIC), (13, 129, 100, 0, GENERIC), (48, 129, 64, 0, GENERIC)]


@pytest.mark.parametrize("k,S,chunk,force,kernel", CHUNKS, ids=["%s-S%d-chunk%d-%s" % (c[0], c[1], c[2], "generic" if c[4] == GENERIC else "k4") for c in CHUNKS])
def test_site_chunks(eng, oracle, k, S, chunk, force, kernel):
    from phyly_amd import engine as E
    wl, codes, ref = _family(oracle, k, S)
    wl.setup_engine(eng)
    wts = cases.weights_with_zeros(S, S + chunk)
    assert np.sum(wts == 0) > 0 and wts[-1] != wts[0]
    label = "%s S=%d chunk=%d kernel %d" % (k, S, chunk, kernel)
    try:
        _set_options(eng, {E.OPT_FORCE_GENERIC: force, E.OPT_SITE_CHUNK: chunk})
        eng.set_patterns_codes(codes, wl.defs)
        chunked = _hold(eng, ref, wts, kernel, label)
        _set_options(eng, {E.OPT_FORCE_GENERIC: force})
        whole = _hold(eng, ref, wts, kernel, label + " (one chunk)")
        assert np.max(np.abs(chunked - whole)) <= 1e-14 * np.max(np.abs(whole)), label      # the same sums in another order
    finally:
        _reset(eng)


# ------------------------------------------------------------------ rescaled nodes above k = 5
def test_rescaled_nodes_k13(eng, oracle):
    """a 40-taxon caterpillar, observation rows scaled by 1e-8: every site likelihood is below 1e-300, so the
    ldexp(inv, XM - XMdiv) reconciliation of k_up carries the result.  The bar is the one
    test_gpu_hess.test_rescaled_passes_tiny_likelihoods uses for this kind of input, 1e-10, for (a) and (b)."""
    md = mixsens_cases.caterpillar_doc(40, 9, seed=13, k=13, C=2, leaf_scale=1e-8)
    try:
        _set_options(eng, {})
        m, w = mixsens_cases.setup_engine(eng, oracle, md)
        assert m.E == 78
        ref = cases.Reference(oracle, m, w, m.B, exact=2)
        assert np.max(ref.ll) < np.log(1e-300), np.max(ref.ll)
        _hold(eng, ref, None, GENERIC, "caterpillar k=13", bar=1e-10)
        _hold(eng, ref, np.linspace(0.5, 1.5, 9), GENERIC, "caterpillar k=13 weighted", bar=1e-10)
    finally:
        _reset(eng)


# ------------------------------------------------------------------ the JSON drivers above k = 8
JSON_WEIGHTS = [round(0.4 + 0.35 * (i % 6), 2) for i in range(33)]
# whether the commands' values count (second_order_cases.counts): 33 sites condition the 22 and 18 rates of the k = 9 and
# k = 17 trees to kappa = 2e6 and 2e4 only, so there the commands are held to "refused or finite"; k = 33 (kappa 2e3) counts
JSON_COUNTS = {9: False, 17: False, 33: True}


@pytest.mark.parametrize("agg", ["sum", "weights"])
@pytest.mark.parametrize("k", [9, 17, 33])
def test_json_path(oracle, k, agg):
    import arbplf
    wl = family_workload(k)
    codes = cases.conserved_codes(wl, 33, 33)
    x = {"model_and_data": wl.json_model(codes), "site_reduction": {"aggregation": "sum" if agg == "sum" else JSON_WEIGHTS}}
    s = json.dumps(x)
    _check_table(json.loads(arbplf.arbplf_hess(s)), json.loads(oracle.arbplf_hess(s)), rel=1e-10)
    counted = cases.check_commands(oracle, x)
    assert counted == JSON_COUNTS[k], k


# ------------------------------------------------------------------ two engines
def test_group(monkeypatch):
    """arbplf-hess with the site patterns split over two engines against one engine, as tests/test_gpu_group.py holds
    aggregated values"""
    import arbplf
    wl = family_workload(13)
    S = 129
    x = {"model_and_data": wl.json_model(cases.conserved_codes(wl, S, S)),
         "site_reduction": {"aggregation": np.linspace(0.5, 1.5, S).tolist()}}
    s = json.dumps(x)
    monkeypatch.delenv("ARBPLF_DEVICES", raising=False)
    one = json.loads(arbplf.arbplf_hess(s))
    monkeypatch.setenv("ARBPLF_DEVICES", "0,0")
    two = json.loads(arbplf.arbplf_hess(s))
    monkeypatch.delenv("ARBPLF_DEVICES", raising=False)
    assert one["columns"] == two["columns"] and len(one["data"]) == len(two["data"]) == wl.E * wl.E
    for a, b in zip(one["data"], two["data"]):
        assert a[:-1] == b[:-1]
        assert abs(a[-1] - b[-1]) <= 1e-14 * max(abs(a[-1]), 1e-3), (a, b)
