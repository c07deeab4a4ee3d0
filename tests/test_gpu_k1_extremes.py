"""GPU: K1 (k_expm_dd, k_dP_dd, k_d2p, the ExpmPost ending, k_build_tables_pt, the Frechet blocks) entry by entry at
extreme branch lengths, and every ll family end to end on sites whose likelihood is one entry of one matrix.

The older bar on K1, max |P - P_oracle| <= 4e-16 at edge rates of 0.02-0.3, cannot see an entry of size 1e-9 (or 1e-130,
a three-step entry on a short branch) that is wrong in its first digit, nor a dropped low word of Qn in k_expm_dd
(5.2e-6 relative at the top of the ladder here at k = 4, below 1e-16 at those lengths).  Models, ladder and cases:
tests/k1_cases.py.  That the oracle's rounded P is a correct rounding on this ladder, and that these sites tell a
transposed P or a neighbouring category: tests/test_k1_reference_cpu.py.  DESIGN.md section 2 records the figures.

Bars: |P - ref| <= 2 ulp(ref) (both are roundings of values good to better than 1e-20: 1 ulp expected, one more for
double rounding); exactly 0 where the reference is exactly 0 and exactly 1 on the diagonal of P = I; row sums within
1e-14; ll, deriv, Hessian and Frechet bars are those of tests/test_gpu_kernel_families.py and tests/test_gpu_hess.py,
with one deviation: the scale of a derivative row of the star, and of the Hessian of a single rung, is at least 1, the
floor of the ll bar (_deriv_err and test_hessian_on_single_entries say why), so that every row of every rung is compared.

The refused inputs (tests/k1_cases.check_cases) go to the engine only after the engine-free plk_check_model_values has
returned PLK_E_ARG for them: none of them reaches a kernel."""
import numpy as np
import pytest

import k1_cases as K
from helpers import oracle_model, rel_err
from test_gpu_kernel_families import GENERIC, MFMA, TOL, VEC, _row_err

pytestmark = pytest.mark.gpu

FUSED = 1
ULPS = 2.0


def _set_options(eng, opts):
    from phyly_amd import engine as E
    defaults = {E.OPT_FORCE_GENERIC: 0, E.OPT_SITE_CHUNK: 0, E.OPT_FUSED_NS: 0, E.OPT_FUSED_ASM: 1, E.OPT_UP_NODES: 2,
                E.OPT_PAIR_TABLES: 1, E.OPT_MFMA: 1, E.OPT_MFMA_NS2: 0}
    for o, v in defaults.items():
        eng.set_option(o, opts.get(o, v))


@pytest.fixture(scope="module")
def eng():
    from phyly_amd.engine import Engine
    e = Engine(0)
    yield e
    _set_options(e, {})
    e.close()


def _ambiguous(ref, nchar):
    """the entry sites with every third leaf observation replaced by an ambiguity row that admits the state"""
    codes = ref.codes.copy()
    wl = ref.wl
    for s in range(0, codes.shape[1], 3):
        e, j = ref.triples[s, 2], ref.triples[s, 1]
        rows = [r for r in range(ref.kk + 1, nchar) if wl.defs[r, j] > 0]
        if rows:
            codes[e, s] = rows[s % len(rows)]
    return codes


class _Ref:
    """oracle values of one (k, mixed) star model, built once: P, the entry sites (with nchar: every third leaf
    observation an ambiguity row), their ll and derivatives"""

    def __init__(self, oracle, k, mixed, nchar=None):
        self.wl = wl = K.star_workload(k, mixed, nchar=nchar)
        self.kk = kk = wl.k
        self.m, self.w = oracle_model(oracle, wl, K.entry_sites(kk, [(0, 0, 0)]))
        self.P = self.w["P"]
        live = self.P[-1]                                        # one category, or the fastest of the mixture
        self.triples = K.all_entries(live) if kk <= 13 else K.some_entries(live, seed=kk)
        self.codes = K.entry_sites(kk, self.triples)
        if nchar is not None:
            self.codes = _ambiguous(self, nchar)
        self.ll, _ = oracle.site_ll(self.m, self.w, codes=np.ascontiguousarray(self.codes.T), defs=wl.defs, precise=2)
        self._oracle, self._deriv = oracle, None

    @property
    def deriv(self):
        if self._deriv is None:
            self._deriv = self._oracle.site_deriv(self.m, self.w, self.wl.defs[self.codes.T], precise=2)
        return self._deriv


_REFS = {}


def _ref(oracle, k, mixed, nchar=None):
    key = (k, mixed, nchar)
    if key not in _REFS:
        _REFS[key] = _Ref(oracle, k, mixed, nchar)
    return _REFS[key]


def _benign(ref, nchar=None):
    """the same model at edge rates 0.1: what the engine holds before plk_update_edge_rates takes it to the ladder"""
    k = "birth" if isinstance(ref.wl, K.BirthWorkload) else ref.kk
    return K.star_workload(k, ref.wl.rate_mixture is not None, nchar=nchar, rates=[0.1] * 12)


def _deriv_err(got, want, edge):
    """-> (worst, worst per edge of the site) of |got - want| / max(row scale, 1) over all rows.  This is the suite's bar
    on derivatives, 1e-12 of max(|value|, row scale), with the floor of its ll bar, max(1, .), and that floor is the one
    deviation from it.  The row of site (i, j, e) holds r dP_ij / P_ij on edge e and exactly 0 on the eleven edges to
    leaves without data, where fp64 returns the rounding of a row sum of dP (1e-17).  Up to the rung 0.1 the value is
    about m / t, the scale is its own and the floor does nothing.  On the long rungs P is at its limit, the true value
    falls to 0 (the binary128 row is its own rounding noise, 1e-34, on the last ones) and nothing computed from a P
    rounded to fp64 can follow it down: there the floor asks that dP_ij / P_ij be 0 to 1e-12 absolutely, which a dP
    that is wrong by more than 1e-12 of P misses."""
    got, want = got.reshape(len(got), -1), want.reshape(len(want), -1)
    err = np.max(np.abs(got - want), axis=1) / np.maximum(np.max(np.abs(want), axis=1), 1.0)
    return float(np.max(err)), [float(np.max(err[edge == e])) if np.any(edge == e) else 0.0 for e in range(12)]


def _compare_P(P, ref, what):
    d = K.ulp_distance(P, ref.P)
    zero = ref.P == 0
    print("%s %s: worst %.2f ulp over %d non-zero entries (smallest %.3g), %d exact zeros"
          % (ref.wl.name, what, np.max(d[~zero]), np.sum(~zero), np.min(ref.P[~zero]), np.sum(zero)))
    assert np.all(P[zero] == 0.0), what
    kk = ref.kk
    eye = np.eye(kk, dtype=bool)
    assert np.all(P[0][:, eye] == 1.0) and np.all(P[:, 0][:, eye] == 1.0), what          # P = I: the rate-0 category, the rate-0 edge
    assert np.max(d) <= ULPS, (what, float(np.max(d)), np.unravel_index(np.argmax(d), d.shape))
    np.testing.assert_allclose(P.sum(axis=-1), 1.0, rtol=0, atol=1e-14)


# ------------------------------------------------------------------ P, entry by entry
@pytest.mark.parametrize("k", [4, 13, 27, 61, "birth"])
def test_transition_matrices_entry_by_entry(eng, oracle, k):
    """LDS product (k <= 26), tiled global product (k >= 27), up to 45 squarings; once after plk_set_model, once after
    plk_set_model at rates 0.1 and plk_update_edge_rates to the ladder (k = 4: with the formats built, so that K1 runs
    with its ExpmPost ending)"""
    ref = _ref(oracle, k, True)
    wl = ref.wl
    k0 = wl.prepare()
    top = np.max(k0["cat_rates"]) * np.max(wl.edge_rates_csr) * K.qnorm(k0["Qn"])
    assert 0.999 * K.LIMIT < top < K.LIMIT
    _set_options(eng, {})
    wl.setup_engine(eng)
    _compare_P(eng.transition_matrices(), ref, "after set_model")
    _benign(ref).setup_engine(eng)
    eng.set_patterns_codes(ref.codes, wl.defs)
    eng.set_site_weights(None)
    eng.ll()
    eng.update_edge_rates(wl.edge_rates_csr)
    eng.ll()
    _compare_P(eng.transition_matrices(), ref, "after update_edge_rates")


# ------------------------------------------------------------------ end to end through every ll family
def _ll_cases():
    """-> [(k, name, options, layout, ll kernel, nchar)]"""
    from phyly_amd import engine as E
    return [(4, "pairs1", {E.OPT_PAIR_TABLES: 1}, "codes", FUSED, None),
            (4, "pairs0", {E.OPT_PAIR_TABLES: 0}, "codes", FUSED, None),
            (4, "generic", {E.OPT_FORCE_GENERIC: 1}, "codes", GENERIC, None),
            (4, "dense", {}, "dense", GENERIC, None),
            (4, "ambiguity", {}, "codes", FUSED, 7),
            (13, "vec", {}, "codes", VEC, None),
            (13, "ambiguity", {}, "codes", VEC, 16),
            (27, "vec", {}, "codes", VEC, None),
            (27, "mfma", {E.OPT_MFMA: 2}, "codes", MFMA, None),
            (61, "mfma", {}, "codes", MFMA, None),
            ("birth", "generic", {}, "codes", GENERIC, None)]


def _case_ids(cases):
    return [pytest.param(c[0], c[1], id="k%s-%s" % (c[0], c[1])) for c in cases]


@pytest.mark.parametrize("mixed", [False, True], ids=["one-category", "mixture"])
@pytest.mark.parametrize("k,case", _case_ids(_ll_cases()))
def test_ll_and_deriv_on_single_entries(eng, oracle, k, case, mixed):
    """plk_ll and plk_deriv on the entry sites, every row of every rung, after set-up and again after
    plk_update_edge_rates from rates 0.1 (for the k = 4 formats: ExpmPost and k_build_tables_pt wrote what the kernel
    reads); the ambiguity cases read P and dP through the double-double P defs of the tip tables"""
    from phyly_amd import engine as E
    _, _, opts, layout, llk, nchar = next(c for c in _ll_cases() if c[:2] == (k, case))
    ref = _ref(oracle, k, mixed, nchar)
    wl = ref.wl
    codes, want = ref.codes, ref.ll
    if nchar is not None:
        assert wl.defs.shape[0] == nchar == ref.kk + 3
        assert np.sum(codes[:12] > ref.kk) >= codes.shape[1] // 6
    assert np.all(np.isfinite(want))

    def load():
        if layout == "dense":
            eng.set_patterns_dense(np.ascontiguousarray(wl.defs[codes].transpose(0, 2, 1)))
        else:
            eng.set_patterns_codes(codes, wl.defs)
        eng.set_site_weights(None)
    try:
        _set_options(eng, opts)
        for path in ("set_model", "update_edge_rates"):
            if path == "set_model":
                wl.setup_engine(eng)
                load()
            else:
                _benign(ref, nchar).setup_engine(eng)
                load()
                eng.ll()
                eng.update_edge_rates(wl.edge_rates_csr)
            got, _ = eng.ll()
            assert eng.info(E.INFO_LL_KERNEL) == llk, (path, eng.info(E.INFO_LL_KERNEL))
            print("%s %s: ll kernel %d variant %d" % (wl.name, case, eng.info(E.INFO_LL_KERNEL), eng.info(E.INFO_LL_VARIANT)))
            if k == 4 and layout == "codes" and llk == FUSED:
                assert eng.info(E.INFO_LL_VARIANT) == (1 if opts.get(E.OPT_PAIR_TABLES, 1) == 0 else 6), (path, eng.info(E.INFO_LL_VARIANT))
            err = rel_err(got, want)
            print("%s %s %s %s: ll rel err %.3g over %d sites" % (wl.name, case, "mixture" if mixed else "one category", path, err, len(want)))
            assert err <= TOL, path
            d, _ = eng.deriv()
            derr, per_rung = _deriv_err(d, ref.deriv, ref.triples[:, 2])
            print("%s %s %s %s: deriv err %.3g over all %d rows; per rung %s"
                  % (wl.name, case, "mixture" if mixed else "one category", path, derr, len(d), " ".join("%.1e" % v for v in per_rung)))
            assert derr <= TOL, (path, per_rung)
    finally:
        eng.set_site_weights(None)
        _set_options(eng, {})


# ------------------------------------------------------------------ cherries with unequal ladder edges
_CHERRY = {}


def _cherry_ref(oracle, k):
    if k not in _CHERRY:
        wl = K.cherry_workload(k, True)
        codes = K.cherry_sites(wl, seed=7700 + k)
        m, w = oracle_model(oracle, wl, codes)
        ll, _ = oracle.site_ll(m, w, codes=np.ascontiguousarray(codes.T), defs=wl.defs, precise=2)
        deriv = oracle.site_deriv(m, w, wl.defs[codes.T], precise=2)
        _CHERRY[k] = (wl, codes, ll, deriv)
    return _CHERRY[k]


@pytest.mark.parametrize("k,pairs,variant", [(4, 1, 6), (4, 5, 6), (4, 6, 6), (4, 0, 1), (13, 1, 0)])
def test_cherries_with_unequal_ladder_edges(eng, oracle, k, pairs, variant):
    """pair-table orientation at the extremes: the two leaf edges of cherry n take rungs n and 11 - n"""
    from phyly_amd import engine as E
    wl, codes, ll, deriv = _cherry_ref(oracle, k)
    assert codes.shape[1] == 65 and sum(np.sum(codes[2 * n] != codes[2 * n + 1]) for n in range(6)) >= 32
    assert np.all(np.isfinite(ll))
    try:
        _set_options(eng, {E.OPT_PAIR_TABLES: pairs})
        wl.setup_engine(eng)
        eng.set_patterns_codes(codes, wl.defs)
        eng.set_site_weights(None)
        got, _ = eng.ll()
        assert eng.info(E.INFO_LL_KERNEL) == (FUSED if k == 4 else VEC)
        assert eng.info(E.INFO_LL_VARIANT) == variant, eng.info(E.INFO_LL_VARIANT)
        assert (eng.info(E.INFO_PAIR_TABLES) > 0) == (pairs != 0)
        err = rel_err(got, ll)
        d, _ = eng.deriv()
        derr = _row_err(d, deriv)
        print("cherries k=%d pairs=%d: ll rel err %.3g, deriv row err %.3g" % (k, pairs, err, derr))
        assert err <= TOL
        assert derr <= TOL
    finally:
        _set_options(eng, {})


# ------------------------------------------------------------------ Frechet blocks
FRECHET_RUNGS = (0.0, 1e-12, 1e-3, 30.0, 1e3)


@pytest.mark.parametrize("k", [4, 13, 14, 32])
def test_frechet_blocks(eng, oracle, k):
    """the 2k x 2k form (LDS for k <= 13, tiled global above) with the three coefficient modes; L in [-1, 1] and the same
    L scaled by 1e6 and 1e-6 (the squaring count follows the larger of s |Qn| and |L|); at t = 0 the block is coef L"""
    from phyly_amd import engine as E
    mixture = K.MIX if k <= 14 else None                         # k = 32: one category keeps the binary128 build short
    wl = K._shell(k, FRECHET_RUNGS, mixture, None, edges=[[5, leaf] for leaf in range(5)])
    codes = np.full((6, 1), k, dtype=np.uint8)
    m, ow = oracle_model(oracle, wl, codes)
    _set_options(eng, {})
    wl.setup_engine(eng)
    L0 = np.random.default_rng(7800 + k).uniform(-1, 1, (k, k))
    for factor in (1.0, 1e6, 1e-6):
        L = L0 * factor
        want0 = oracle.frechet(m, ow, L, 1.0, False, None, precise=1).reshape(ow["C"], wl.E, k, k)
        for coef in (E.COEF_PRIOR, E.COEF_PRIOR_RATE_EDGE, E.COEF_PRIOR_RATE):
            got = eng.frechet_matrices(L, coef)
            want = want0.copy()
            for c in range(ow["C"]):
                for e in range(wl.E):
                    if coef == E.COEF_PRIOR_RATE_EDGE:
                        want[c, e] *= ow["cat_rates"][c] * m.edge_rates_csr[e]
                    elif coef == E.COEF_PRIOR_RATE:
                        want[c, e] *= ow["cat_rates"][c]
            scale = np.max(np.abs(want), axis=(2, 3), keepdims=True)
            err = np.max(np.abs(got - want) / np.maximum(scale, 1e-300))
            print("frechet k=%d L x %g coef %d: %.3g of the largest entry" % (k, factor, coef, err))
            assert err <= 1e-14, (factor, coef)
            e0 = int(np.flatnonzero(np.asarray(m.edge_rates_csr) == 0.0)[0])
            for c in range(ow["C"]):
                cf = 1.0 if coef == E.COEF_PRIOR else (0.0 if coef == E.COEF_PRIOR_RATE_EDGE else ow["cat_rates"][c])
                assert np.max(np.abs(got[c, e0] - cf * L)) <= 1e-14 * np.max(np.abs(cf * L)), (factor, coef, c)


# ------------------------------------------------------------------ k_d2p
HESS_RUNGS = (1e-6, 1e-3, 0.1, 30.0)


def _hess_case(oracle, k, rates):
    """-> (workload, codes, oracle Hessian summed over the sites) of 64 seeded single-entry sites on the star"""
    wl = K.star_workload(k, False, rates=rates)
    m, ow = oracle_model(oracle, wl, K.entry_sites(k, [(0, 0, 0)]))
    triples = K.all_entries(ow["P"][0])
    triples = triples[np.random.default_rng(7900 + k).choice(len(triples), 64, replace=False)]
    codes = K.entry_sites(k, triples)
    want = oracle.site_hess(m, ow, wl.defs[codes.T], precise=2).astype(np.longdouble).sum(axis=0).astype(float)
    return wl, codes, want


@pytest.mark.parametrize("k", [4, 13])
def test_hessian_on_single_entries(eng, oracle, k):
    """plk_hess (k_d2p: d2P = r^2 Qn^2 P) on 64 single-entry sites, one category, the rungs 1e-6, 1e-3, 0.1 and 30: once
    with the four rungs on one star (three edges each), at 1e-11 of the largest entry, which the rung 1e-6 sets at about
    1e12, so that this call pins the short rungs only; then one star per rung, all twelve edges on it, at
    1e-11 max(largest entry, 1), which gives each rung its own scale (about 1e12, 1e6, 1e3; on the rung 30 the entries
    are at most 1, P is at its limit and the floor is that of the ll bar: the sum over the sites of the second
    derivatives of log P_ij is 0 to 1e-11 absolutely)"""
    _set_options(eng, {})
    for rung in (None,) + HESS_RUNGS:
        wl, codes, want = _hess_case(oracle, k, list(HESS_RUNGS) * 3 if rung is None else [rung] * 12)
        wl.setup_engine(eng)
        eng.set_patterns_codes(codes, wl.defs)
        eng.set_site_weights(None)
        got = eng.hess()
        largest = np.max(np.abs(want))
        err = np.max(np.abs(got - want)) / (largest if rung is None else max(largest, 1.0))
        print("hess k=%d %s: %.3g of %s (largest entry %.3g)"
              % (k, "four rungs" if rung is None else "rung %g" % rung, err, "the largest entry" if rung is None else "max(largest entry, 1)", largest))
        assert np.allclose(got, got.T, rtol=0, atol=0), rung
        assert err <= 1e-11, rung


# ------------------------------------------------------------------ refusals
REFUSED = [c for c in K.check_cases() if c[1] and len(c[2]["Qn"]) == 3 and len(c[2]["er"]) == 3]


@pytest.mark.parametrize("name", [c[0] for c in REFUSED])
def test_refused_values_leave_the_engine_as_it_was(eng, name):
    """every refused input is first refused by the engine-free check; only then does it go to plk_set_model, to
    plk_update_edge_rates followed by plk_ll (its edge rates), and, where one of its values is not finite, to
    plk_get_frechet_matrices as a direction; after each refusal an ll on the valid model gives its earlier bits"""
    from phyly_amd import engine as E
    from phyly_amd.engine import EngineError
    _, _, v, names = next(c for c in REFUSED if c[0] == name)
    assert E.check_model_values(v["Qn"], v["er"], v["cr"], v["cp"], v["root_mode"], v["rw"], Qn_lo=v["Qn_lo"]) == E.E_ARG
    good = K.check_cases()[0][2]
    assert E.check_model_values(good["Qn"], good["er"], good["cr"], good["cp"], good["root_mode"], good["rw"], Qn_lo=good["Qn_lo"]) == 0
    indptr, indices, preorder, _ = __import__("phyly_amd.synth", fromlist=["synth"]).csr_from_edges([[3, 0], [3, 1], [3, 2]])
    _set_options(eng, {})
    eng.set_tree(indptr, indices, preorder)
    eng.set_model(good["Qn"], good["er"], good["cr"], good["cp"], good["root_mode"], good["rw"], Qn_lo=good["Qn_lo"])
    codes = np.array([[0, 1, 2, 3, 0], [1, 1, 0, 2, 3], [2, 0, 1, 3, 3], [3, 3, 3, 3, 1]], dtype=np.uint8)
    defs = np.vstack([np.eye(3), np.ones((1, 3))])
    eng.set_patterns_codes(codes, defs)
    eng.set_site_weights(None)
    before, _ = eng.ll()
    assert np.all(np.isfinite(before))

    def refused(call):
        with pytest.raises(EngineError) as err:
            call()
        assert err.value.code == E.E_ARG, str(err.value)
        if names is not None:
            assert "edge %d " % names[0] in str(err.value) and "category %d " % names[1] in str(err.value)
        after, _ = eng.ll()
        assert np.array_equal(before, after)

    refused(lambda: eng.set_model(v["Qn"], v["er"], v["cr"], v["cp"], v["root_mode"], v["rw"], Qn_lo=v["Qn_lo"]))
    assert (eng.k, eng.C) == (3, 2)
    if E.check_model_values(good["Qn"], v["er"], good["cr"], good["cp"], good["root_mode"], good["rw"], Qn_lo=good["Qn_lo"]) == E.E_ARG:
        names = None
        refused(lambda: eng.update_edge_rates(v["er"]))
    if not np.all(np.isfinite(v["Qn"])):
        L = np.array(v["Qn"])
        assert not np.all(np.isfinite(L))
        for coef in (E.COEF_PRIOR, E.COEF_PRIOR_RATE_EDGE, E.COEF_PRIOR_RATE):
            refused(lambda: eng.frechet_matrices(L, coef))
        refused(lambda: eng.frechet_matrices(np.zeros((3, 3)), E.COEF_PRIOR, L_lo=L))
        refused(lambda: eng.edge_expect(L, E.COEF_PRIOR))
