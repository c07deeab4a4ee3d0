"""GPU: every k = 4 kernel variant against the oracle on asymmetric models (helpers.K4_MODELS).

The other engine-level k = 4 tests force their variants on synth.Workload gtr_g4 / hky85: a reversible Q under the
equilibrium root prior, gamma categories of equal prior and positive rate, strictly binary trees without data on internal
nodes, positive site weights.  The four models here have a non-reversible Q and between them every root prior, a rate-0
category, unequal category priors, a rate-0 edge, a unary node, multifurcations, data on a cherry parent and on another
internal node, a data-free cherry whose two edge rates differ 7.5 x (the orientation of a pair table), 7 and 17 character
definitions (4-bit and 8-bit staged codes), stack needs 4 (the pair-table limit) and 5, and C = 1, 2, 4 and 5 categories
(C = 5 leaves the node-visit up pass and the k = 4 second-order pass).  tests/test_kernel_family_models.py shows on the CPU
that these models tell a wrong kernel from a right one.

Oracle values (binary128, precise = 2) are built once per model.  Site counts are one past every tile size (256, 512,
1024, 1536) with a ragged last wave; a model runs the sizes its variants can tile.  Every case asserts the kernel, the
variant and the up-pass path it ran on (PLK_INFO_LL_KERNEL, PLK_INFO_LL_VARIANT, PLK_INFO_PAIR_TABLES,
PLK_INFO_UPDOWN_KERNEL, PLK_INFO_UP4_PATH) against what plk_k4_choose (plk_program.h) and run_updown4
prescribe for the model, so an option or dispatch change cannot quietly move a case off the path its name claims.

Tolerances and weights are those of tests/test_gpu_kernel_families.py."""
import numpy as np
import pytest

from helpers import (IRREGULAR_CHERRY, IRREGULAR_EDGES, IRREGULAR_RATES, K4_MODELS, cherry_with_unequal_edges, deep_workload, family_workload,
                     k4_workload, oracle_model, rel_err, tree_workload)
from second_order_cases import edge_scale, scaled_err
from test_gpu_kernel_families import MFMA, PROB_ULP, SUM_TOL, TOL, VEC, _row_err, _wsum

gpu = pytest.mark.gpu                # every test but the one on the tables of expected paths, which needs no GPU

FUSED, GENERIC, HESS4 = 1, 2, 5
# PLK_INFO_UP4_PATH bits
NODES, PAIRS, REBUILD, INLINE = 1, 2, 4, 8

# stack need, categories, character definitions of each model.  Every ll case asserts slots and C against the engine's info
# items; no info item gives the engine's nchar, so the case asserts it on the definitions it hands to the engine, and
# that the data of "wide" use codes >= 16, which do not fit the 4-bit staged form
# (the irregular tree is two caterpillars and a leaf under the root: one waiting vector)
SHAPE = {"irregular": dict(slots=1, C=4, nchar=7), "balanced32": dict(slots=4, C=1, nchar=5),
         "balanced64": dict(slots=5, C=5, nchar=5), "wide": dict(slots=1, C=2, nchar=17)}
# the pair-table interpreters tile 512, 1024 or 1536 sites; models beyond their limits (4 slots, 16 definitions) only
# ever run 256-site tiles
LL_SIZES = {"irregular": (1, 65, 257, 513, 1025, 1601), "balanced32": (1, 65, 257, 513, 1025, 1601),
            "balanced64": (1, 65, 257, 513), "wide": (1, 65, 257, 513)}
UD_SIZES = (1, 65, 257)              # UD4_BLOCK = 256
XS = 65                              # edge expectations
# second order: the oracle's binary128 Hessian (precise = 2, the call of test_gpu_hess.test_engine_matches_oracle for k = 4)
# costs E^2 entries per site and category; balanced64 has E = 126 and C = 5 (43 s for 65 sites on one core), so there it
# covers one partial wave, the first 5 of the 65 sites.  The 65 sites themselves (one site past GEN_BLOCK) are compared
# with the oracle's long-double Hessian (precise = 1, 3 s), which _Ref first holds against the binary128 one on those 5
# sites to 1e-14 of the largest entry: three decades inside the 1e-11 bar, which stays
HESS_SIZES = {"irregular": (65, 257), "balanced32": (65, 257), "balanced64": (5, 65)}
HESS_LONG_DOUBLE = {("balanced64", 65)}
HESS_SCALED = ("irregular", "balanced32")      # also held entry by entry at the scale d_i d_j of second_order_cases.edge_scale


def _pt(model):
    s = SHAPE[model]
    return s["slots"] <= 4 and s["nchar"] <= 16


def _ll_cases(model):
    """-> [(name, options, layout, ll kernel, variant, pair tables > 0)]: the option tuples of test_gpu_fused_asm._both
    (and PLK_OPT_PAIR_TABLES = 6, the 1536-site tile), two sites per lane, forced generic, the dense layout.
    plk_k4_choose: pair tables need PLK_OPT_FUSED_ASM, one site per lane, <= 4 slots, <= 16 definitions; option 1 / 5 / 6
    give the two-sites-per-lane interpreter (variant 6), 2 / 3 the one-site one (variant 5).  Without them
    then the assembly interpreter where it fits (variant 1; up to 8 slots, one site per lane), else the C++ one (3)."""
    from phyly_amd import engine as E
    pt = _pt(model)
    out = []
    for pairs, variant in ((1, 6), (5, 6), (6, 6), (2, 5), (3, 5)):
        out.append(("pairs%d" % pairs, {E.OPT_PAIR_TABLES: pairs}, "codes", FUSED, variant if pt else 1, pt))
    out.append(("asm", {E.OPT_PAIR_TABLES: 0}, "codes", FUSED, 1, False))
    out.append(("cpp", {E.OPT_PAIR_TABLES: 0, E.OPT_FUSED_ASM: 0}, "codes", FUSED, 3, False))
    out.append(("cpp-pairs-on", {E.OPT_FUSED_ASM: 0}, "codes", FUSED, 3, False))
    out.append(("cpp-two-sites", {E.OPT_FUSED_NS: 2}, "codes", FUSED, 3, False))
    out.append(("generic", {E.OPT_FORCE_GENERIC: 1}, "codes", GENERIC, 0, False))
    out.append(("dense", {}, "dense", GENERIC, 0, False))
    return out


def _ud_cases(model):
    """-> [(name, options, up/down kernel, PLK_INFO_UP4_PATH of a derivative query)].  run_updown4: the node-visit pass
    takes derivative queries of models with at most 4 categories under PLK_OPT_UP_NODES bit 1; pair messages need
    PLK_OPT_PAIR_TABLES, <= 16 definitions and a data-free cherry (every model has one); rebuilt tables (a data-free node
    over two leaves or pair nodes: every model has one) go with bit 2 clear; the inline form needs pair messages, C = 1
    and bit 3 clear.  Marginal and expectation queries always take k_up4 (path 0)."""
    from phyly_amd import engine as E
    s = SHAPE[model]
    out = []
    for up in (2, 0, 6, 10):
        for pairs in (1, 0):
            path = 0
            if (up & 2) and s["C"] <= 4:
                pm = bool(pairs) and s["nchar"] <= 16
                path = NODES | (PAIRS if pm else 0) | (0 if up & 4 else REBUILD) | (INLINE if pm and s["C"] == 1 and not up & 8 else 0)
            out.append(("up%d-pairs%d" % (up, pairs), {E.OPT_UP_NODES: up, E.OPT_PAIR_TABLES: pairs}, FUSED, path))
    out.append(("generic", {E.OPT_FORCE_GENERIC: 1}, GENERIC, 0))
    return out


def test_expected_paths_cover_every_up_pass_form():
    """the table above reaches every combination the node-visit pass has: plain, pair messages, rebuilt tables, both,
    and the inline form with and without rebuilt tables"""
    seen = {c[3] for mdl in K4_MODELS for c in _ud_cases(mdl)}
    assert seen == {0, NODES, NODES | REBUILD, NODES | PAIRS, NODES | PAIRS | REBUILD, NODES | PAIRS | INLINE,
                    NODES | PAIRS | REBUILD | INLINE}


_DEFAULTS = None


def _set_options(eng, opts):
    from phyly_amd import engine as E
    global _DEFAULTS
    if _DEFAULTS is None:
        _DEFAULTS = {E.OPT_FORCE_GENERIC: 0, E.OPT_SITE_CHUNK: 0, E.OPT_FUSED_NS: 0, E.OPT_FUSED_ASM: 1, E.OPT_UP_NODES: 2,
                     E.OPT_PAIR_TABLES: 1, E.OPT_MFMA: 1, E.OPT_MFMA_NS2: 0}
    for o, v in _DEFAULTS.items():
        eng.set_option(o, opts.get(o, v))


def _reset(eng):
    eng.set_site_weights(None)
    _set_options(eng, {})


@pytest.fixture(scope="module")
def eng():
    from phyly_amd.engine import Engine
    e = Engine(0)
    yield e
    _set_options(e, {})
    e.close()


def _weights(S):
    rng = np.random.default_rng(S + 7)
    return rng.choice([-1.0, 1.0], S) * 10.0 ** rng.uniform(-3, 3, S)


class _Ref:
    """oracle values of one model, built once"""

    def __init__(self, oracle, model):
        self.model = model
        self.wl = wl = k4_workload(model)
        sizes = LL_SIZES[model]
        self.data = {S: (wl.simulate(S) if i % 2 == 0 else wl.random_codes(S, seed=S, missing_frac=0.1)) for i, S in enumerate(sizes)}
        self.m, self.w = oracle_model(oracle, wl, self.data[1])
        self.ll, self.deriv, self.marg = {}, {}, {}
        for S, codes in self.data.items():
            self.ll[S], _ = oracle.site_ll(self.m, self.w, codes=np.ascontiguousarray(codes.T), defs=wl.defs, precise=2)
        for S in UD_SIZES:
            B = wl.defs[self.data[S].T]
            self.deriv[S] = oracle.site_deriv(self.m, self.w, B, precise=2)
            self.marg[S] = oracle.site_marginal(self.m, self.w, B, precise=2)
        rng = np.random.default_rng(44)
        self.Ls = rng.uniform(-1, 1, (4, 4, 4))
        self.xmask = np.zeros(wl.E, dtype=np.int32)
        self.xmask[rng.choice(wl.E, size=5, replace=False)] = 1
        B = wl.defs[self.data[XS].T]
        self.expect = {}
        for d in range(4):
            F = oracle.frechet(self.m, self.w, self.Ls[d], 1.0, False, self.xmask, precise=2)
            for coef in ((0, 1) if d == 0 else (1,)):
                self.expect[d, coef] = oracle.site_edge_expect(self.m, self.w, B, F, coef, self.xmask, precise=2)
        self.hess, self.hscale = {}, {}
        self.hdata, self.hderiv = {}, {}
        for S in HESS_SIZES.get(model, ()):
            src = S if S in self.deriv else 65
            self.hdata[S], self.hderiv[S] = np.ascontiguousarray(self.data[src][:, :S]), self.deriv[src][:S]
            wts = np.linspace(0.5, 1.5, S)
            H = oracle.site_hess(self.m, self.w, wl.defs[self.hdata[S].T], precise=1 if (model, S) in HESS_LONG_DOUBLE else 2)
            if (model, S) in HESS_LONG_DOUBLE:
                exact = site_hess_5                                   # binary128, the same first sites
                assert np.max(np.abs(H[:5] - exact)) <= 1e-14 * np.max(np.abs(exact))
            elif S == 5:
                site_hess_5 = H
            self.hess[S] = (H.astype(np.longdouble) * wts[:, None, None].astype(np.longdouble)).sum(axis=0).astype(float)
            self.hscale[S] = edge_scale(H, self.hderiv[S], wts)            # each edge's own curvature, for the scaled bar


_REFS = {}


@pytest.fixture
def ref(oracle, request):
    model = request.node.callspec.params["model"]
    if model not in _REFS:
        _REFS[model] = _Ref(oracle, model)
    return _REFS[model]


def _params(cases):
    return [pytest.param(mdl, c[0], id="%s-%s" % (mdl, c[0])) for mdl in K4_MODELS for c in cases(mdl)]


def _case(cases, model, name):
    return next(c for c in cases(model) if c[0] == name)


# ------------------------------------------------------------------ ll
@gpu
@pytest.mark.parametrize("model,case", _params(_ll_cases))
def test_ll(eng, ref, model, case):
    from phyly_amd import engine as E
    _, opts, layout, llk, variant, pairs = _case(_ll_cases, model, case)
    wl = ref.wl
    wl.setup_engine(eng)
    nchar = SHAPE[model]["nchar"]
    assert wl.defs.shape == (nchar, 4)
    try:
        _set_options(eng, opts)
        for S, codes in ref.data.items():
            want = ref.ll[S]
            assert codes.max() < nchar and (nchar <= 16 or S < 65 or np.sum(codes >= 16) >= 10), S
            if layout == "dense":
                eng.set_patterns_dense(np.ascontiguousarray(wl.defs[codes].transpose(0, 2, 1)))      # [N][k][S]
            else:
                eng.set_patterns_codes(codes, wl.defs)
            eng.set_site_weights(None)
            got, (hi, lo) = eng.ll()
            assert eng.info(E.INFO_LL_KERNEL) == llk, S
            assert eng.info(E.INFO_LL_VARIANT) == variant, (S, eng.info(E.INFO_LL_VARIANT))
            assert (eng.info(E.INFO_PAIR_TABLES) > 0) == pairs, S
            assert eng.info(E.INFO_STACK_SLOTS) == SHAPE[model]["slots"] and eng.info(E.INFO_CATEGORIES) == SHAPE[model]["C"]
            assert rel_err(got, want) <= TOL, S
            assert abs((hi + lo) - float(np.sum(want.astype(np.longdouble)))) <= TOL * np.sum(np.abs(want)), S
            wts = _weights(S)
            eng.set_site_weights(wts)
            got, (hi, lo) = eng.ll()
            assert eng.info(E.INFO_LL_VARIANT) == variant, S
            assert rel_err(got, want) <= TOL, S
            bound = SUM_TOL * float(np.sum(np.abs(wts) * np.maximum(1.0, np.abs(want))))
            assert abs((hi + lo) - float(_wsum(want, wts))) <= bound, S
    finally:
        _reset(eng)


@gpu
@pytest.mark.parametrize("model", ["irregular", "balanced32"])
def test_cherry_orientation_is_visible(ref, model):
    """the data the pair-table cases run on hold sites where the two leaves of the data-free cherry with the most
    unequal edges show different codes: a pair table read as [code_c][code_b] moves their ll
    (tests/test_kernel_family_models.py shows it on the CPU)"""
    b, c = cherry_with_unequal_edges(ref.wl)
    if model == "irregular":
        assert {b, c} == set(IRREGULAR_CHERRY)
    for S, codes in ref.data.items():
        if S >= 65:
            assert np.sum(codes[b] != codes[c]) >= 10, S


# ------------------------------------------------------------------ deriv, marginal, edge expectations
@gpu
@pytest.mark.parametrize("model,case", _params(_ud_cases))
def test_deriv(eng, ref, model, case):
    from phyly_amd import engine as E
    _, opts, udk, path = _case(_ud_cases, model, case)
    wl = ref.wl
    wl.setup_engine(eng)
    mask = np.zeros(wl.E, dtype=np.int32)
    mask[[0, wl.E // 2, wl.E - 1]] = 1
    sel = mask.astype(bool)
    try:
        _set_options(eng, opts)
        for S in UD_SIZES:
            want = ref.deriv[S]
            eng.set_patterns_codes(ref.data[S], wl.defs)
            wts = _weights(S)
            eng.set_site_weights(wts)
            got, sums = eng.deriv()
            assert eng.info(E.INFO_UPDOWN_KERNEL) == udk, S
            assert eng.info(E.INFO_UP4_PATH) == path, (S, eng.info(E.INFO_UP4_PATH))
            assert _row_err(got, want) <= TOL, S
            scale = np.max(np.abs(want), axis=1)
            bound = SUM_TOL * np.sum(np.abs(wts) * scale)
            assert np.max(np.abs((sums[:, 0] + sums[:, 1]) - _wsum(want, wts).astype(float))) <= bound, S
            got, sums = eng.deriv(edge_mask=mask)
            assert eng.info(E.INFO_UP4_PATH) == path, S
            assert _row_err(got[:, sel], want[:, sel]) <= TOL, S
            assert np.all(got[:, ~sel] == 0.0) and np.all(sums[~sel] == 0.0), S
        # site chunks that are not a multiple of the block: chunks start off the fused down pass's alignment
        eng.set_option(E.OPT_SITE_CHUNK, 100)
        S = 257
        eng.set_patterns_codes(ref.data[S], wl.defs)
        eng.set_site_weights(None)
        got, _ = eng.deriv()
        assert eng.info(E.INFO_UPDOWN_KERNEL) == udk and eng.info(E.INFO_UP4_PATH) == path
        assert _row_err(got, ref.deriv[S]) <= TOL
    finally:
        _reset(eng)


@gpu
@pytest.mark.parametrize("model,case", _params(_ud_cases))
def test_marginal(eng, ref, model, case):
    from phyly_amd import engine as E
    _, opts, udk, _ = _case(_ud_cases, model, case)
    wl = ref.wl
    wl.setup_engine(eng)
    mask = (np.arange(wl.N) % 3 == 0).astype(np.int32)
    sel = mask.astype(bool)
    try:
        _set_options(eng, opts)
        for S in UD_SIZES:
            want = ref.marg[S]
            eng.set_patterns_codes(ref.data[S], wl.defs)
            wts = _weights(S)
            eng.set_site_weights(wts)
            got, sums = eng.marginal()
            assert eng.info(E.INFO_UPDOWN_KERNEL) == udk and eng.info(E.INFO_UP4_PATH) == 0, S
            assert np.max(np.abs(got - want)) <= TOL, S
            ref_sum = _wsum(want, wts).astype(float)
            bound = SUM_TOL * _wsum(np.abs(want), np.abs(wts)).astype(float) + PROB_ULP * np.sum(np.abs(wts))
            assert np.all(np.abs((sums[..., 0] + sums[..., 1]) - ref_sum) <= bound), S
            _, fused = eng.marginal(per_site=False)                # summed as the up pass produces them
            assert eng.info(E.INFO_UPDOWN_KERNEL) == udk, S
            assert np.all(np.abs((fused[..., 0] + fused[..., 1]) - ref_sum) <= bound), S
            got, sums = eng.marginal(node_mask=mask)
            assert np.max(np.abs(got[:, sel] - want[:, sel])) <= TOL, S
            assert np.all(got[:, ~sel] == 0.0) and np.all(sums[~sel] == 0.0), S
        eng.set_option(E.OPT_SITE_CHUNK, 100)
        S = 257
        eng.set_patterns_codes(ref.data[S], wl.defs)
        eng.set_site_weights(None)
        got, _ = eng.marginal()
        assert np.max(np.abs(got - ref.marg[S])) <= TOL
    finally:
        _reset(eng)


@gpu
@pytest.mark.parametrize("model,case", _params(_ud_cases))
def test_edge_expect(eng, ref, model, case):
    """both coefficient modes for one direction; 2, 3 and 4 directions per pass (k_up4<true, false, 2 | 3 | 4>) against
    single calls and the oracle.  Forced generic: several directions are split into single passes."""
    from phyly_amd import engine as E
    _, opts, udk, _ = _case(_ud_cases, model, case)
    wl = ref.wl
    wl.setup_engine(eng)
    sel = ref.xmask.astype(bool)
    try:
        _set_options(eng, opts)
        eng.set_patterns_codes(ref.data[XS], wl.defs)
        eng.set_site_weights(None)
        single = {}
        for d, coef, mode in ((0, 0, E.COEF_PRIOR), (0, 1, E.COEF_PRIOR_RATE_EDGE), (1, 1, E.COEF_PRIOR_RATE_EDGE),
                              (2, 1, E.COEF_PRIOR_RATE_EDGE), (3, 1, E.COEF_PRIOR_RATE_EDGE)):
            want = ref.expect[d, coef]
            got, sums = eng.edge_expect(ref.Ls[d], mode, edge_mask=ref.xmask)
            assert eng.info(E.INFO_UPDOWN_KERNEL) == udk and eng.info(E.INFO_UP4_PATH) == 0, (d, mode)
            assert _row_err(got[:, sel], want[:, sel]) <= TOL, (d, mode)
            assert np.all(got[:, ~sel] == 0.0), (d, mode)
            tot = (sums[:, 0] + sums[:, 1])[sel]
            bound = SUM_TOL * np.sum(np.max(np.abs(want[:, sel]), axis=1))
            assert np.max(np.abs(tot - want[:, sel].astype(np.longdouble).sum(axis=0).astype(float))) <= bound, (d, mode)
            single[d, coef] = (got, sums)
        for nL in (2, 3, 4):
            got, sums = eng.edge_expect_multi(ref.Ls[:nL], E.COEF_PRIOR_RATE_EDGE, edge_mask=ref.xmask)
            assert eng.info(E.INFO_UPDOWN_KERNEL) == udk, nL
            for d in range(nL):
                assert np.array_equal(got[:, d, :], single[d, 1][0]), (nL, d)
                assert np.array_equal(sums[d], single[d, 1][1]), (nL, d)
                assert _row_err(got[:, d, :][:, sel], ref.expect[d, 1][:, sel]) <= TOL, (nL, d)
    finally:
        _reset(eng)


# ------------------------------------------------------------------ second order
@gpu
@pytest.mark.parametrize("force_generic", [0, 1])
@pytest.mark.parametrize("model", ["irregular", "balanced32", "balanced64"])
def test_second_order(eng, ref, model, force_generic):
    """plk_second_order and plk_hess against the oracle call and bar of test_gpu_hess.test_engine_matches_oracle; models
    with at most 4 categories must report the k = 4 pass, balanced64 (C = 5) the generic one"""
    from phyly_amd import engine as E
    wl = ref.wl
    wl.setup_engine(eng)
    want_kernel = HESS4 if SHAPE[model]["C"] <= 4 and not force_generic else GENERIC
    try:
        _set_options(eng, {E.OPT_FORCE_GENERIC: force_generic})
        for S in HESS_SIZES[model]:
            want = ref.hess[S]
            wts = np.linspace(0.5, 1.5, S)
            eng.set_patterns_codes(ref.hdata[S], wl.defs)
            eng.set_site_weights(wts)
            grad, H2 = eng.second_order()
            assert eng.info(E.INFO_UPDOWN_KERNEL) == want_kernel, S
            H1 = eng.hess()
            assert eng.info(E.INFO_UPDOWN_KERNEL) == want_kernel, S
            for got in (H1, H2):
                assert np.allclose(got, got.T, rtol=0, atol=0), S
                assert np.max(np.abs(got - want)) <= 1e-11 * np.max(np.abs(want)), S
                if model in HESS_SCALED:
                    assert np.all(ref.hscale[S] > 0), S
                    assert scaled_err(got, want, ref.hscale[S]) <= 1e-11, (S, scaled_err(got, want, ref.hscale[S]))
            gwant = _wsum(ref.hderiv[S], wts).astype(float)
            scale = np.max(np.abs(ref.hderiv[S]), axis=1)
            assert np.max(np.abs(grad - gwant)) <= TOL * np.sum(np.abs(wts) * scale), S       # the per-site tolerance, summed
    finally:
        _reset(eng)


# ------------------------------------------------------------------ a site of likelihood zero under a zero weight
def _zero_site_workload(k):
    """-> (workload, codes, site): rate 0 on both edges of a cherry whose two leaves agree at every site except `site`,
    where they show states 0 and 1: likelihood exactly 0.  k = 4: the irregular tree and its cherry (0, 1); larger k:
    the model of helpers.FAMILY_MODELS and the first cherry of its tree"""
    if k == 4:
        rates = list(IRREGULAR_RATES)
        for i, (_, child) in enumerate(IRREGULAR_EDGES):
            if child in IRREGULAR_CHERRY:
                rates[i] = 0.0
        wl = tree_workload(4, IRREGULAR_EDGES, rates, root="custom", seed=4401, nchar=7, data_nodes=(18, 17),
                           rate_mixture=dict(rates=[0.0, 0.4, 1.1, 2.7], prior=[0.15, 0.4, 0.05, 0.4]))
        b, c = IRREGULAR_CHERRY
    else:
        wl = family_workload(k)
        leaf = wl.indptr[1:] == wl.indptr[:-1]
        a = next(a for a in range(wl.N) if wl.indptr[a + 1] - wl.indptr[a] == 2 and all(leaf[wl.indices[wl.indptr[a]:wl.indptr[a + 1]]]))
        e0 = wl.indptr[a]
        b, c = int(wl.indices[e0]), int(wl.indices[e0 + 1])
        wl.edge_rates_csr = np.array(wl.edge_rates_csr, dtype=float)
        wl.edge_rates_csr[e0:e0 + 2] = 0.0               # the engine and the simulator read the CSR order; no oracle here
        wl._cum = None
    codes = wl.simulate(40)
    if k != 4:
        codes[a] = k                                     # the cherry's parent shows the missing code: some models put data there
    codes[c] = codes[b]
    codes[b, 7], codes[c, 7] = 0, 1
    return wl, codes, 7


def _ld(s):
    s = np.asarray(s)
    return s[..., 0].astype(np.longdouble) + s[..., 1].astype(np.longdouble)


def _zero_cases():
    """-> (k, name, options, ll kernel, up/down kernel): the k = 4 kernels, and one case per kernel family whose site sums
    mask a zero weight: the vector kernels (k = 20), the matrix-core kernels with one (k = 20, 61) and two (k = 61) site
    groups per workgroup, the generic kernels"""
    from phyly_amd import engine as E
    return [(4, "fused", {}, FUSED, FUSED), (4, "generic", {E.OPT_FORCE_GENERIC: 1}, GENERIC, GENERIC),
            (20, "vec", {}, VEC, VEC), (20, "mfma", {E.OPT_MFMA: 2}, MFMA, MFMA),
            (61, "mfma", {}, MFMA, MFMA), (61, "mfma-ns2", {E.OPT_MFMA_NS2: 1}, MFMA, MFMA)]


@gpu
@pytest.mark.parametrize("k,case", [pytest.param(c[0], c[1], id="k%d-%s" % c[:2]) for c in _zero_cases()])
def test_zero_likelihood_site_under_zero_weight(eng, k, case):
    """ll, deriv and marginal sums (two-stage and fused) with weight 0 on a site of likelihood 0: either the `site
    likelihood zero` error or finite sums equal to those of the alignment without the site; never NaN or inf"""
    from phyly_amd import engine as E
    from phyly_amd.engine import EngineError
    _, _, opts, llk, udk = next(c for c in _zero_cases() if c[:2] == (k, case))
    wl, codes, site = _zero_site_workload(k)
    S = codes.shape[1]
    keep = [s for s in range(S) if s != site]
    wt = np.ones(S)
    wt[site] = 0.0
    queries = {"ll": lambda: np.asarray([eng.ll(per_site=False)[1]]),
               "deriv": lambda: eng.deriv(per_site=False)[1],
               "marginal two-stage": lambda: eng.marginal()[1],
               "marginal fused": lambda: eng.marginal(per_site=False)[1]}
    wl.setup_engine(eng)
    try:
        _set_options(eng, opts)
        eng.set_patterns_codes(codes, wl.defs)
        eng.set_site_weights(None)
        ll, _ = eng.ll()
        assert not np.isfinite(ll[site]) and np.all(np.isfinite(ll[keep]))              # the site is what the name says
        assert eng.info(E.INFO_LL_KERNEL) == llk
        eng.set_site_weights(wt)
        got = {}
        for name, q in queries.items():
            try:
                got[name] = _ld(q())
            except EngineError as err:
                assert "site likelihood zero" in str(err), name
        assert eng.info(E.INFO_UPDOWN_KERNEL) == udk
        eng.set_patterns_codes(np.ascontiguousarray(codes[:, keep]), wl.defs)
        eng.set_site_weights(None)
        for name, q in queries.items():
            if name not in got:
                continue
            want = _ld(q())
            assert np.all(np.isfinite(got[name].astype(float))), name
            err = float(np.max(np.abs(got[name] - want)) / np.max(np.abs(want)))
            assert err <= 1e-14, (name, err)
    finally:
        _reset(eng)


# ------------------------------------------------------------------ the 16-slot C++ interpreter
@gpu
def test_ll_sixteen_slot_interpreter(eng, oracle):
    """k_ll_fused4<16, 1> on the only kind of input that reaches it.  Its LDS image fits with one character definition
    only, and every internal node then shows that definition too: unless it is the all-ones row, all 1535 nodes are
    staged rows and the tile no longer fits.  So the alignment is all-missing, every partial vector is 1 and
    ll = log(sum of the root weights) at every site.  Such data cannot tell a wrong traversal from a right one (a
    waiting vector popped from the wrong slot is 1 as well); what this pins is that the dispatch reaches the
    instantiation (kernel 1, variant 3, 9 slots), that it launches with 144 KiB of LDS and 16 parked vectors in two tiles,
    and that the scalings on the way up and the custom root prior end in the right number."""
    from phyly_amd import engine as E
    wl = deep_workload()
    wl.setup_engine(eng)
    try:
        _set_options(eng, {})
        S = 257
        codes = np.zeros((wl.N, S), dtype=np.uint8)
        m, w = oracle_model(oracle, wl, codes)
        want, _ = oracle.site_ll(m, w, codes=np.ascontiguousarray(codes[:, :1].T), defs=wl.defs, precise=2)
        assert abs(want[0] - np.log(np.sum(wl.root_custom))) <= 1e-14
        eng.set_patterns_codes(codes, wl.defs)
        eng.set_site_weights(None)
        got, (hi, lo) = eng.ll()
        assert eng.info(E.INFO_LL_KERNEL) == FUSED and eng.info(E.INFO_LL_VARIANT) == 3
        assert eng.info(E.INFO_STACK_SLOTS) == 9 and eng.info(E.INFO_PAIR_TABLES) == 0
        assert rel_err(got, np.full(S, want[0])) <= TOL
        assert abs((hi + lo) - S * want[0]) <= TOL * S * abs(want[0])
    finally:
        _reset(eng)
