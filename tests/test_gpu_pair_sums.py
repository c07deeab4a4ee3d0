"""GPU: plk_edge_pair_sums against the binary128 oracle (tests/qgrad_cases.py) and against the engine's own site-summed
queries that are contractions of W.  The accuracy figures each test prints go into DESIGN.md next to their bounds."""
import ctypes

import numpy as np
import pytest

import qgrad_cases as cases
from phyly_amd import engine as E_, synth
from phyly_amd.engine import Engine, EngineError, load_library

pytestmark = pytest.mark.gpu
LD = np.longdouble


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _ld(x):
    return np.asarray(x[..., 0], dtype=LD) + np.asarray(x[..., 1], dtype=LD)


def _weights(S, seed):
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.1, 3.0, S)
    w[rng.random(S) < 0.15] = 0.0
    return w


def _check(name, got, want, tol):
    """per (category, edge): |got - want| <= tol * max|want[c][e]|"""
    scale = np.max(np.abs(want), axis=(-2, -1), keepdims=True) if want.ndim == 4 else np.max(np.abs(want), axis=-1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(scale > 0, np.abs(got - want) / scale, np.abs(got - want))
    worst = float(np.max(rel))
    print("%s: worst error %.3g of max|.| per (c, e) (bound %.0e)" % (name, worst, tol))
    assert np.all(np.isfinite(np.asarray(got, dtype=float))) and worst <= tol, name


def _run_case(eng, oracle, md, kernel, seed, force_generic=False, factored=False):
    eng.set_option(E_.OPT_FORCE_GENERIC, 1 if force_generic else 0)
    try:
        m, w = cases.setup_engine(eng, oracle, md)
        wt = _weights(m.S, seed)
        eng.set_site_weights(wt)
        W, R = eng.edge_pair_sums()
        assert eng.info(E_.INFO_PAIR_SUMS_KERNEL) == kernel
        W2, R2 = eng.edge_pair_sums()
        assert np.array_equal(W, W2) and np.array_equal(R, R2)            # fixed summation order
        want = (cases.oracle_W_factored if factored else cases.oracle_W)(oracle, m, w, wt)
        name = "k=%d C=%d S=%d kernel %d" % (m.k, int(w["C"]), m.S, kernel)
        _check(name + " W", _ld(W), want, 1e-12)
        _check(name + " root", _ld(R), cases.oracle_root(oracle, m, w, wt, per_category=True), 1e-12)
    finally:
        eng.set_option(E_.OPT_FORCE_GENERIC, 0)
        eng.set_site_weights(None)


@pytest.mark.parametrize("C", [4, 1])
@pytest.mark.parametrize("S", [1, 63, 257, 1000])
def test_k4_kernel_against_oracle(eng, oracle, S, C):
    _run_case(eng, oracle, cases.nine_taxon_doc(S, C, seed=100 + S + C), 1, seed=S)


@pytest.mark.parametrize("how", ["force_generic", "dense"])
def test_generic_kernel_on_the_k4_inputs(eng, oracle, how):
    md = cases.nine_taxon_doc(257, 4, seed=361, dense=how == "dense")
    _run_case(eng, oracle, md, 2, seed=5, force_generic=how == "force_generic")


@pytest.mark.parametrize("k,C,S", [(2, 4, 130), (5, 4, 130), (8, 1, 65), (4, 5, 257)])
def test_generic_kernel_small_state_counts(eng, oracle, k, C, S):
    _run_case(eng, oracle, cases.nine_taxon_doc(S, C, seed=500 + k + C, k=k), 2, seed=k)


@pytest.mark.parametrize("k", [20, 61])
def test_generic_kernel_large_state_counts(eng, oracle, k):
    """k^2 binary128 up passes are out of reach here: the oracle's W comes from 2k + 1 calls per category
    (qgrad_cases.oracle_W_factored, checked against the k^2-call form in tests/test_rate_matrix_chain_host.py)"""
    _run_case(eng, oracle, cases.small_tree_doc(65, k, seed=600 + k, T=3 if k == 61 else 4), 2, seed=k, factored=True)


def test_600_taxon_tiny_likelihoods(eng, oracle):
    """the 600-taxon generator of tests/test_gpu_hess.py: site likelihoods below the double range, rescaled vectors"""
    wl = synth.Workload(T=600, k=4, tree="yule", model="gtr_g4", seed=17)
    wl.setup_engine(eng)
    codes = wl.random_codes(64, seed=4, missing_frac=0.02)
    eng.set_patterns_codes(codes, wl.defs)
    eng.set_site_weights(None)
    ll, _ = eng.ll()
    assert np.max(ll) < -745
    W, _ = eng.edge_pair_sums()
    assert eng.info(E_.INFO_PAIR_SUMS_KERNEL) == 1
    m = oracle.parse_model(wl.json_model(codes))
    w = oracle.prepare(m)
    want = cases.oracle_W(oracle, m, w, np.ones(64), cats=[2])
    _check("600 taxa, category 2", _ld(W)[2], want[2], 1e-12)


@pytest.fixture(scope="module")
def cfg3(eng):
    wl = synth.Workload(3)
    wl.setup_engine(eng)
    S = 20000
    codes = wl.simulate(S)
    eng.set_patterns_codes(codes, wl.defs)
    wt = _weights(S, 3)
    eng.set_site_weights(wt)
    eng.set_option(E_.OPT_SITE_CHUNK, 0)
    W, R = eng.edge_pair_sums()
    yield wl, codes, wt, _ld(W), _ld(R)
    eng.set_site_weights(None)


def test_cfg3_contractions(eng, cfg3):
    """<W, dP> summed over categories is the plk_deriv edge sum; <W, P> is the summed posterior of the category, on every edge"""
    wl, codes, wt, W, R = cfg3
    assert eng.info(E_.INFO_PAIR_SUMS_KERNEL) == 1
    ll0, s0 = eng.ll()
    _, dsum = eng.deriv(per_site=False)
    dsum = _ld(dsum)
    P = eng.transition_matrices().astype(LD)
    k0 = wl.prepare()
    Qn = np.asarray(k0["Qn"], dtype=LD) + np.asarray(k0["Qn_lo"], dtype=LD)
    dP = np.einsum("c,ij,cejl->ceil", np.asarray(k0["cat_rates"], dtype=LD), Qn, P)
    got = np.einsum("ceij,ceij->e", W, dP)
    err = float(np.max(np.abs(got - dsum)) / np.max(np.abs(dsum)))
    _, _, psum, _ = eng.cat_posterior(per_site=False)
    psum = _ld(psum)
    post = np.einsum("ceij,ceij->ce", W, P)
    perr = float(np.max(np.abs(post - psum[:, None])) / np.sum(wt))
    print("cfg3 20000 sites: <W, dP> vs plk_deriv %.3g of max|edge sum| (bound 1e-11); <W, P> vs post_sums %.3g of sum w (bound 1e-11)" % (err, perr))
    assert err <= 1e-11 and perr <= 1e-11
    # no disturbance: plk_ll and plk_deriv give the same bits after the call as before
    eng.edge_pair_sums()
    ll1, s1 = eng.ll()
    _, dsum1 = eng.deriv(per_site=False)
    assert np.array_equal(ll0, ll1) and s0 == s1 and np.array_equal(_ld(dsum1), dsum)


def test_cfg3_chunked_equals_unchunked(eng, cfg3):
    wl, codes, wt, W, R = cfg3
    eng.set_option(E_.OPT_SITE_CHUNK, 4096)
    try:
        Wc, Rc = eng.edge_pair_sums()
    finally:
        eng.set_option(E_.OPT_SITE_CHUNK, 0)
    err = float(np.max(np.abs(_ld(Wc) - W) / np.maximum(np.abs(W), 1e-300)))
    rerr = float(np.max(np.abs(_ld(Rc) - R) / np.abs(R)))
    print("cfg3 chunked (4096) vs unchunked: W %.3g, root %.3g relative (bound 1e-13)" % (err, rerr))
    assert err <= 1e-13 and rerr <= 1e-13


def test_cfg3_group_of_two_equals_one_engine(cfg3):
    wl, codes, wt, W, R = cfg3
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
    lib.plk_group_edge_pair_sums.argtypes = [vp, vp, vp, vp]
    k0 = wl.prepare()
    C, S = k0["C"], codes.shape[1]
    P = lambda a: a.ctypes.data_as(vp)
    g = vp()
    assert lib.plk_group_create(ctypes.byref(g), 2, (ci * 2)(0, 0)) == 0
    try:
        ip, ix, pre = (np.ascontiguousarray(a, dtype=np.int32) for a in (wl.indptr, wl.indices, wl.preorder))
        assert lib.plk_group_set_tree(g, wl.N, P(ip), P(ix), P(pre)) == 0
        Qn, Ql, er = (np.ascontiguousarray(a, dtype=np.float64) for a in (k0["Qn"], k0["Qn_lo"], wl.edge_rates_csr))
        cr, cp, pi = (np.ascontiguousarray(a, dtype=np.float64) for a in (k0["cat_rates"], k0["cat_prior"], k0["pi"]))
        assert lib.plk_group_set_model(g, wl.k, C, P(Qn), P(Ql), P(er), P(cr), P(cp), 4, P(pi)) == 0
        defs = np.ascontiguousarray(wl.defs, dtype=np.float64)
        cd = np.ascontiguousarray(codes)
        assert lib.plk_group_set_patterns_codes(g, S, P(cd), wl.nchar, P(defs)) == 0, lib.plk_group_last_error(g)
        assert lib.plk_group_set_site_weights(g, P(np.ascontiguousarray(wt))) == 0
        Wg, Rg = np.zeros((C, wl.E, 4, 4, 2)), np.zeros((C, 4, 2))
        assert lib.plk_group_edge_pair_sums(g, None, P(Wg), P(Rg)) == 0, lib.plk_group_last_error(g)
    finally:
        lib.plk_group_destroy(g)
    err = float(np.max(np.abs(_ld(Wg) - W) / np.maximum(np.abs(W), 1e-300)))
    rerr = float(np.max(np.abs(_ld(Rg) - R) / np.abs(R)))
    print("cfg3 group (0, 0) vs one engine: W %.3g, root %.3g relative (bound 1e-13)" % (err, rerr))
    assert err <= 1e-13 and rerr <= 1e-13


@pytest.mark.parametrize("force_generic", [0, 1])
def test_edge_mask(eng, oracle, force_generic):
    eng.set_option(E_.OPT_FORCE_GENERIC, force_generic)
    try:
        m, w = cases.setup_engine(eng, oracle, cases.nine_taxon_doc(257, 4, seed=71))
        eng.set_site_weights(None)
        W, _ = eng.edge_pair_sums()
        mask = np.array([(e * 7 + 3) % 3 != 0 for e in range(m.E)], dtype=np.int32)
        Wm, _ = eng.edge_pair_sums(edge_mask=mask)
    finally:
        eng.set_option(E_.OPT_FORCE_GENERIC, 0)
    assert np.all(Wm[:, mask == 0] == 0) and np.any(mask == 0)
    assert np.array_equal(Wm[:, mask != 0], W[:, mask != 0])


@pytest.mark.parametrize("force_generic", [0, 1])
def test_zero_likelihood_site(eng, oracle, force_generic):
    """site 7 shows two different states at the cherry (4, 5) whose edges have rate 0: likelihood exactly 0"""
    md = cases.nine_taxon_doc(40, 4, seed=72)
    md["edge_rate_coefficients"][3] = md["edge_rate_coefficients"][4] = 0.0        # edges 1 -> 4 and 1 -> 5
    for row in md["character_data"]:
        row[5] = row[4] if row[4] < 4 else 0
        row[4] = row[5]
    md["character_data"][7][4], md["character_data"][7][5] = 0, 1
    eng.set_option(E_.OPT_FORCE_GENERIC, force_generic)
    try:
        cases.setup_engine(eng, oracle, md)
        eng.set_site_weights(None)
        with pytest.raises(EngineError, match="site likelihood zero"):
            eng.edge_pair_sums()
        with pytest.raises(EngineError, match="site likelihood zero"):
            eng.rate_matrix_sens()
        wt = np.ones(40)
        wt[7] = 0.0
        eng.set_site_weights(wt)
        W, R = eng.edge_pair_sums()
        assert np.all(np.isfinite(W)) and np.all(np.isfinite(R)) and np.max(W) > 0
    finally:
        eng.set_option(E_.OPT_FORCE_GENERIC, 0)
        eng.set_site_weights(None)
