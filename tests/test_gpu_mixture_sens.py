"""GPU: plk_mixture_sens against the oracle expectations of tests/mixsens_cases.py, its identities with plk_deriv and
plk_cat_posterior, determinism, isolation, chunking, zero-likelihood sites and the group call.  Every case is run once
(module cache) and shared by the tests that look at it.  The figures each test prints go into DESIGN.md."""
import ctypes

import numpy as np
import pytest

import mixsens_cases as cases
from phyly_amd import engine as E_
from phyly_amd.engine import Engine, EngineError, load_library

pytestmark = pytest.mark.gpu
LD = np.longdouble

# name -> (document builder, kernel the engine must report).  Shapes: the smallest at which each kernel can go wrong.
CASES = {
    "k4_C1": (lambda: cases.five_taxon_doc(70, 1, seed=11), 1),              # 70 sites: two waves, the last partial
    "k4_C4": (lambda: cases.five_taxon_doc(70, 4, seed=12), 1),              # a category of rate 0, one of prior 0
    "k4_rescale": (lambda: cases.caterpillar_doc(40, 70, seed=13, leaf_scale=1e-8), 1),
    "k4_C5_generic": (lambda: cases.five_taxon_doc(70, 5, seed=14), 2),      # Gamma4 + I: more than 4 categories
    "k4_dense_generic": (lambda: cases.five_taxon_doc(70, 4, seed=12, dense=True), 2),
    "k20_generic": (lambda: cases.caterpillar_doc(6, 40, seed=15, k=20, C=4), 2),
    "k61_generic": (lambda: cases.caterpillar_doc(4, 10, seed=16, k=61, C=2), 2),
}
_cache = {}


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _ld(x):
    return np.asarray(x[..., 0], dtype=LD) + np.asarray(x[..., 1], dtype=LD)


def _weights(S, seed):
    w = np.random.default_rng(seed).uniform(0.1, 3.0, S)      # non-integer
    w[S // 3] = 0.0
    w[S // 2] = 2.0
    return w


def _run(eng, oracle, name):
    if name in _cache:
        return _cache[name]
    build, kernel = CASES[name]
    md = build()
    m, w = cases.setup_engine(eng, oracle, md)
    wt = _weights(m.S, len(name))
    eng.set_site_weights(wt)
    try:
        # isolation: the other queries before ...
        ll0, s0 = eng.ll()
        _, d0 = eng.deriv(per_site=False)
        _, _, ps0, _ = eng.cat_posterior(per_site=False)
        po, ro = eng.mixture_sens()
        got_kernel = eng.info(E_.INFO_MIXTURE_SENS_KERNEL)
        po2, ro2 = eng.mixture_sens()
        # ... and after
        ll1, s1 = eng.ll()
        _, d1 = eng.deriv(per_site=False)
        _, _, ps1, _ = eng.cat_posterior(per_site=False)
    finally:
        eng.set_site_weights(None)
    r = dict(md=md, m=m, w=w, k0=cases.product_k0(m), wt=wt, po=po, ro=ro, po2=po2, ro2=ro2, kernel=got_kernel, want_kernel=kernel,
             same=np.array_equal(ll0, ll1) and s0 == s1 and np.array_equal(d0, d1) and np.array_equal(ps0, ps1),
             dsum=_ld(d0), psum=_ld(ps0))
    _cache[name] = r
    return r


@pytest.mark.parametrize("name", list(CASES))
def test_against_oracle(eng, oracle, name):
    """bar: 1e-12 of max_c |value| (the project's bar for site-summed forms); the rate of a category of rate 0 is held to
    the accuracy of its forward difference instead (mixsens_cases.expectations)"""
    r = _run(eng, oracle, name)
    assert r["kernel"] == r["want_kernel"]
    want_p, want_r, tol_r = cases.expectations(oracle, r["md"], r["wt"])
    if name == "k4_rescale":
        ll, _ = oracle.site_ll(r["m"], r["w"], B=r["m"].B, precise=2)
        assert np.max(ll) < np.log(1e-300)                    # only a rescaling pass gets through these sites
    got_p, got_r = _ld(r["po"]), _ld(r["ro"])
    assert np.all(np.isfinite(r["po"])) and np.all(np.isfinite(r["ro"]))
    ep = np.abs(got_p - want_p) / np.max(np.abs(want_p))
    er = np.abs(got_r - want_r) / np.max(np.abs(want_r))
    exact = tol_r == 0
    print("%s (kernel %d): prior_out %.3g, rate_out %.3g of max|.| (bound 1e-12); rate-0 category %.3g (bound %.3g)"
          % (name, r["kernel"], float(np.max(ep)), float(np.max(er[exact])) if np.any(exact) else 0.0,
             float(np.max(er[~exact])) if np.any(~exact) else 0.0, float(np.max(tol_r))))
    assert np.all(ep <= 1e-12)
    assert np.all(er <= np.maximum(tol_r, LD(1e-12)))


@pytest.mark.parametrize("name", list(CASES))
def test_identities(eng, oracle, name):
    """sum_c p_c prior_out[c] = sum_s w_s; sum_c r_c rate_out[c] = sum_e t_e (plk_deriv edge sums);
    p_c prior_out[c] = post_sums[c] of plk_cat_posterior -- all to 1e-13 relative"""
    r = _run(eng, oracle, name)
    p, rate = np.asarray(r["k0"]["cat_prior"], dtype=LD), np.asarray(r["k0"]["cat_rates"], dtype=LD)      # what the engine was given
    got_p, got_r = _ld(r["po"]), _ld(r["ro"])
    sw = np.sum(np.asarray(r["wt"], dtype=LD))
    e1 = float(abs(np.sum(p * got_p) - sw) / sw)
    t = np.asarray(r["m"].edge_rates_csr, dtype=LD)
    rhs = np.sum(t * r["dsum"])
    scale = max(np.max(np.abs(rate * got_r)), abs(rhs))        # the terms cancel: relative to the largest of them
    e2 = float(abs(np.sum(rate * got_r) - rhs) / scale)
    e3 = float(np.max(np.abs(p * got_p - r["psum"])) / sw)
    print("%s: sum p prior_out vs sum w %.3g; sum r rate_out vs sum t deriv %.3g; p prior_out vs post_sums %.3g (bound 1e-13)" % (name, e1, e2, e3))
    assert e1 <= 1e-13 and e2 <= 1e-13 and e3 <= 1e-13


@pytest.mark.parametrize("name", list(CASES))
def test_determinism_and_isolation(eng, oracle, name):
    r = _run(eng, oracle, name)
    assert np.array_equal(r["po"], r["po2"]) and np.array_equal(r["ro"], r["ro2"])      # fixed summation order
    assert r["same"]                              # plk_ll, plk_deriv, plk_cat_posterior: the same bits before and after


@pytest.mark.parametrize("C,kernel", [(4, 1), (5, 2)])
def test_chunked_equals_unchunked(eng, oracle, C, kernel):
    """300 sites in chunks of 256: a chunk boundary changes the grid of partial sums, so 1e-14 relative, not bits"""
    md = cases.five_taxon_doc(300, C, seed=21)
    cases.setup_engine(eng, oracle, md)
    eng.set_site_weights(_weights(300, 2))
    try:
        po, ro = eng.mixture_sens()
        eng.set_option(E_.OPT_SITE_CHUNK, 256)
        pc, rc = eng.mixture_sens()
        assert eng.info(E_.INFO_MIXTURE_SENS_KERNEL) == kernel
    finally:
        eng.set_option(E_.OPT_SITE_CHUNK, 0)
        eng.set_site_weights(None)
    ep = float(np.max(np.abs(_ld(pc) - _ld(po))) / np.max(np.abs(_ld(po))))
    er = float(np.max(np.abs(_ld(rc) - _ld(ro))) / np.max(np.abs(_ld(ro))))
    print("C=%d chunked (256 of 300) vs unchunked: prior_out %.3g, rate_out %.3g of max|.| (bound 1e-14)" % (C, ep, er))
    assert ep <= 1e-14 and er <= 1e-14


@pytest.mark.parametrize("force_generic", [0, 1])
def test_zero_likelihood_site(eng, oracle, force_generic):
    """site 7 shows two different states at the cherry (4, 5) whose edges both have rate 0: likelihood exactly 0"""
    md = cases.five_taxon_doc(40, 4, seed=31)
    md["edge_rate_coefficients"][3] = md["edge_rate_coefficients"][4] = 0.0
    for row in md["character_data"]:
        row[5] = row[4]
    md["character_data"][7][4], md["character_data"][7][5] = 0, 1
    eng.set_option(E_.OPT_FORCE_GENERIC, force_generic)
    try:
        cases.setup_engine(eng, oracle, md)
        eng.set_site_weights(None)
        with pytest.raises(EngineError, match="site likelihood zero"):
            eng.mixture_sens()
        wt = np.ones(40)
        wt[7] = 0.0
        eng.set_site_weights(wt)
        po, ro = eng.mixture_sens()
        assert eng.info(E_.INFO_MIXTURE_SENS_KERNEL) == (2 if force_generic else 1)
        assert np.all(np.isfinite(po)) and np.all(np.isfinite(ro))
        # the site contributes nothing: the same sums as on the 39 other sites alone
        keep = [s for s in range(40) if s != 7]
        md39 = dict(md, character_data=[md["character_data"][s] for s in keep])
        cases.setup_engine(eng, oracle, md39)
        eng.set_site_weights(None)
        p39, r39 = eng.mixture_sens()
        ep = float(np.max(np.abs(_ld(po) - _ld(p39))) / np.max(np.abs(_ld(p39))))
        er = float(np.max(np.abs(_ld(ro) - _ld(r39))) / np.max(np.abs(_ld(r39))))
        assert ep <= 1e-14 and er <= 1e-14
    finally:
        eng.set_option(E_.OPT_FORCE_GENERIC, 0)
        eng.set_site_weights(None)


def test_group_of_two_equals_one_engine(eng, oracle):
    md = cases.five_taxon_doc(300, 4, seed=41)
    m, w = cases.setup_engine(eng, oracle, md)
    wt = _weights(300, 5)
    eng.set_site_weights(wt)
    try:
        po, ro = eng.mixture_sens()
    finally:
        eng.set_site_weights(None)
    lib = load_library()
    vp, ci, cl = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    lib.plk_group_create.argtypes = [ctypes.POINTER(vp), ci, vp]
    lib.plk_group_destroy.argtypes = [vp]
    lib.plk_group_destroy.restype = None
    lib.plk_group_last_error.argtypes = [vp]
    lib.plk_group_last_error.restype = ctypes.c_char_p
    lib.plk_group_set_tree.argtypes = [vp, ci, vp, vp, vp]
    lib.plk_group_set_model.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp, ci, vp]
    lib.plk_group_set_patterns_codes.argtypes = [vp, cl, vp, ci, vp]
    lib.plk_group_set_site_weights.argtypes = [vp, vp]
    lib.plk_group_mixture_sens.argtypes = [vp, vp, vp]
    k0 = cases.product_k0(m)
    C = k0["C"]
    P = lambda a: a.ctypes.data_as(vp)
    g = vp()
    assert lib.plk_group_create(ctypes.byref(g), 2, (ci * 2)(0, 0)) == 0
    try:
        ip, ix, pre = (np.ascontiguousarray(a, dtype=np.int32) for a in (m.indptr, m.indices, m.preorder))
        assert lib.plk_group_set_tree(g, m.N, P(ip), P(ix), P(pre)) == 0
        Qn, Ql, er = (np.ascontiguousarray(a, dtype=np.float64) for a in (k0["Qn"], k0["Qn_lo"], m.edge_rates_csr))
        cr, cp, pi = (np.ascontiguousarray(a, dtype=np.float64) for a in (k0["cat_rates"], k0["cat_prior"], k0["pi"]))
        assert lib.plk_group_set_model(g, m.k, C, P(Qn), P(Ql), P(er), P(cr), P(cp), 4, P(pi)) == 0
        defs = np.ascontiguousarray(md["character_definitions"], dtype=np.float64)
        cd = np.ascontiguousarray(np.asarray(md["character_data"], dtype=np.uint8).T)
        assert lib.plk_group_set_patterns_codes(g, 300, P(cd), defs.shape[0], P(defs)) == 0, lib.plk_group_last_error(g)
        assert lib.plk_group_set_site_weights(g, P(np.ascontiguousarray(wt))) == 0
        pg, rg = np.zeros((C, 2)), np.zeros((C, 2))
        assert lib.plk_group_mixture_sens(g, P(pg), P(rg)) == 0, lib.plk_group_last_error(g)
    finally:
        lib.plk_group_destroy(g)
    ep = float(np.max(np.abs(_ld(pg) - _ld(po))) / np.max(np.abs(_ld(po))))
    er = float(np.max(np.abs(_ld(rg) - _ld(ro))) / np.max(np.abs(_ld(ro))))
    print("group (0, 0) vs one engine: prior_out %.3g, rate_out %.3g of max|.| (bound 1e-14)" % (ep, er))
    assert ep <= 1e-14 and er <= 1e-14
