"""GPU: every kernel instance for 5 <= k <= 64 against the oracle on non-reversible models with several rate categories.

One model per state count (helpers.FAMILY_MODELS: non-symmetric Q with a few zero rates, C = 2..4 gamma categories, some
with the rate-0 category, every root prior, ambiguity codes, data on internal nodes).  The oracle's reference values
are built once per state count (module cache); every kernel family that takes that k is forced through the engine
options and checked against them, at site counts that straddle every block size (GEN_BLOCK = MF_SITES = 64, 128 with
PLK_OPT_MFMA_NS2 and UDV_BLOCK, VEC_BLOCK = UD4_BLOCK = 256).  Each case asserts which family ran
(PLK_INFO_LL_KERNEL, PLK_INFO_UPDOWN_KERNEL), so a dispatch change cannot move it onto another path unnoticed.

Tolerances as in BASELINE.md section 2: ll 1e-12 * max(1, |ll|); deriv and edge expectations 1e-12 of the row scale;
marginal 1e-12 absolute.  Site sums use signed weights spread over six decades and are compared with the long-double sum
of the oracle's per-site values to 1e-13 * sum_s |w_s| * v_s, where v_s is the size the per-site tolerance refers to
(|ll_s| or 1 for ll, the row scale for deriv and edge expectations): the per-site values may differ from the oracle's by
rounding at that scale, so a column that is small at a site does not tighten its own bound.  Marginal sums: PROB_ULP."""
import json
import random

import numpy as np
import pytest

from helpers import FAMILY_MODELS, custom_workload, family_workload, nonreversible_rates, oracle_model, rel_err

pytestmark = pytest.mark.gpu

KS = sorted(FAMILY_MODELS)
TOL = 1e-12
SUM_TOL = 1e-13
PROB_ULP = 1e-15    # marginal site sums: 1e-13 * sum_s |w_s v_s| (the fp64 in-wave sum of the fused path stays far inside it,
                    # 64 terms cost at most 64 eps of that), plus 1e-15 * sum_s |w_s| for the absolute rounding each per-site
                    # probability carries at the scale of 1, which a state with a small probability does not shrink
VEC, MFMA, GENERIC = 4, 3, 2


def _families(k):
    """-> [(name, {option: value}, ll kernel, up/down kernel)] for every kernel family that takes k"""
    from phyly_amd import engine as E
    if k <= 8:
        return [("default", {}, GENERIC, GENERIC)]
    out = []
    if k <= 20:
        out += [("vec", {}, VEC, VEC),
                ("vec-no-reg-stack", {E.OPT_VEC_REG_STACK: 0}, VEC, VEC),
                ("vec-no-pair-tables", {E.OPT_PAIR_TABLES: 0}, VEC, VEC),
                ("mfma", {E.OPT_MFMA: 2}, MFMA, MFMA),
                ("mfma-up-nodes", {E.OPT_MFMA: 2, E.OPT_UP_NODES: 3}, MFMA, MFMA)]
    elif k <= 32:
        out += [("vec", {}, VEC, MFMA),
                ("vec-no-pair-tables", {E.OPT_PAIR_TABLES: 0}, VEC, MFMA),
                ("mfma", {E.OPT_MFMA: 2}, MFMA, MFMA),
                ("mfma-up-nodes", {E.OPT_UP_NODES: 3}, VEC, MFMA)]
    else:
        out += [("mfma", {}, MFMA, MFMA),
                ("mfma-ns2", {E.OPT_MFMA_NS2: 1}, MFMA, MFMA),
                ("mfma-up-nodes", {E.OPT_UP_NODES: 3}, MFMA, MFMA)]
    out.append(("generic", {E.OPT_FORCE_GENERIC: 1}, GENERIC, GENERIC))
    return out


def _sizes(k):
    """(S, data kind): S = 129 is two MFMA site groups of a 128-site workgroup and one site past UDV_BLOCK"""
    return [(1, "simulated"), (65, "random"), (257, "simulated")] + ([(129, "random")] if k >= 9 else [])


_DEFAULTS = None


def _set_options(eng, opts):
    from phyly_amd import engine as E
    global _DEFAULTS
    if _DEFAULTS is None:
        _DEFAULTS = {E.OPT_FORCE_GENERIC: 0, E.OPT_SITE_CHUNK: 0, E.OPT_MFMA: 1, E.OPT_UP_NODES: 2, E.OPT_PAIR_TABLES: 1,
                     E.OPT_VEC_REG_STACK: 1, E.OPT_MFMA_NS2: 0}
    for o, v in _DEFAULTS.items():
        eng.set_option(o, opts.get(o, v))


def _reset(eng):
    _set_options(eng, {})


@pytest.fixture(scope="module")
def eng():
    from phyly_amd.engine import Engine
    e = Engine(0)
    yield e
    _reset(e)
    e.close()


class _Ref:
    """oracle values of one state count's model, built once"""

    def __init__(self, oracle, k):
        self.k = k
        self.wl = wl = family_workload(k)
        self.precise = 2 if k <= 8 else 1
        self.data = {}
        for S, kind in _sizes(k):
            codes = wl.simulate(S) if kind == "simulated" else wl.random_codes(S, seed=S, missing_frac=0.1)
            self.data[S] = codes
        self.m, self.w = oracle_model(oracle, wl, self.data[1])
        self.ll, self.deriv, self.marg = {}, {}, {}
        for S, codes in self.data.items():
            B = wl.defs[codes.T]
            self.ll[S], _ = oracle.site_ll(self.m, self.w, codes=np.ascontiguousarray(codes.T), defs=wl.defs,
                                           precise=self.precise)
            self.deriv[S] = oracle.site_deriv(self.m, self.w, B, precise=self.precise)
            self.marg[S] = oracle.site_marginal(self.m, self.w, B, precise=self.precise)
        # conditional edge expectations for one dense direction on two or three edges
        rng = np.random.default_rng(k)
        self.L = rng.uniform(-1, 1, (k, k))
        self.xmask = np.zeros(wl.E, dtype=np.int32)
        self.xmask[rng.choice(wl.E, size=2 if k >= 48 else 3, replace=False)] = 1
        F = oracle.frechet(self.m, self.w, self.L, 1.0, False, self.xmask, precise=self.precise)
        self.xS = 129 if k >= 9 else 65
        B = wl.defs[self.data[self.xS].T]
        self.expect = {c: oracle.site_edge_expect(self.m, self.w, B, F, c, self.xmask, precise=self.precise) for c in (0, 1)}

    def weights(self, S):
        rng = np.random.default_rng(S + 7)
        return rng.choice([-1.0, 1.0], S) * 10.0 ** rng.uniform(-3, 3, S)


_REFS = {}


@pytest.fixture
def ref(oracle, request):
    k = request.node.callspec.params["k"]
    if k not in _REFS:
        _REFS[k] = _Ref(oracle, k)          # a few MB for all k together
    return _REFS[k]


def _cases():
    return [pytest.param(k, f[0], id="k%d-%s" % (k, f[0])) for k in KS for f in _families(k)]


def _family(k, name):
    return next(f for f in _families(k) if f[0] == name)


def _row_err(got, want):
    got = got.reshape(got.shape[0], -1)
    want = want.reshape(want.shape[0], -1)
    scale = np.max(np.abs(want), axis=1, keepdims=True)
    return np.max(np.abs(got - want) / np.maximum(np.abs(want), np.maximum(scale, 1e-300)))


def _wsum(v, w):
    return (v.astype(np.longdouble) * w.reshape((-1,) + (1,) * (v.ndim - 1)).astype(np.longdouble)).sum(axis=0)


@pytest.mark.parametrize("k,family", _cases())
def test_ll(eng, ref, k, family):
    from phyly_amd import engine as E
    _, opts, llk, _ = _family(k, family)
    wl = ref.wl
    wl.setup_engine(eng)
    try:
        _set_options(eng, opts)
        for S, codes in ref.data.items():
            want = ref.ll[S]
            eng.set_patterns_codes(codes, wl.defs)
            eng.set_site_weights(None)
            got, (hi, lo) = eng.ll()
            assert eng.info(E.INFO_LL_KERNEL) == llk, S
            assert rel_err(got, want) <= TOL, S
            assert abs((hi + lo) - float(np.sum(want.astype(np.longdouble)))) <= TOL * np.sum(np.abs(want)), S
            wts = ref.weights(S)
            eng.set_site_weights(wts)
            got, (hi, lo) = eng.ll()
            assert rel_err(got, want) <= TOL, S
            bound = SUM_TOL * float(np.sum(np.abs(wts) * np.maximum(1.0, np.abs(want))))
            assert abs((hi + lo) - float(_wsum(want, wts))) <= bound, S
    finally:
        eng.set_site_weights(None)
        _reset(eng)


@pytest.mark.parametrize("k,family", _cases())
def test_deriv(eng, ref, k, family):
    from phyly_amd import engine as E
    _, opts, _, udk = _family(k, family)
    wl = ref.wl
    wl.setup_engine(eng)
    mask = np.zeros(wl.E, dtype=np.int32)
    mask[[0, wl.E // 2, wl.E - 1]] = 1
    sel = mask.astype(bool)
    try:
        _set_options(eng, opts)
        for S, codes in ref.data.items():
            want = ref.deriv[S]
            eng.set_patterns_codes(codes, wl.defs)
            wts = ref.weights(S)
            eng.set_site_weights(wts)
            got, sums = eng.deriv()
            assert eng.info(E.INFO_UPDOWN_KERNEL) == udk, S
            assert _row_err(got, want) <= TOL, S
            scale = np.max(np.abs(want), axis=1)
            bound = SUM_TOL * np.sum(np.abs(wts) * scale)
            assert np.max(np.abs((sums[:, 0] + sums[:, 1]) - _wsum(want, wts).astype(float))) <= bound, S
            got, sums = eng.deriv(edge_mask=mask)
            assert _row_err(got[:, sel], want[:, sel]) <= TOL, S
            assert np.all(got[:, ~sel] == 0.0) and np.all(sums[~sel] == 0.0), S
        # site chunks that are not a multiple of any kernel's block
        eng.set_option(E.OPT_SITE_CHUNK, 100)
        S = 257
        eng.set_patterns_codes(ref.data[S], wl.defs)
        eng.set_site_weights(None)
        got, _ = eng.deriv()
        assert eng.info(E.INFO_UPDOWN_KERNEL) == udk
        assert _row_err(got, ref.deriv[S]) <= TOL
    finally:
        eng.set_site_weights(None)
        _reset(eng)


@pytest.mark.parametrize("k,family", _cases())
def test_marginal(eng, ref, k, family):
    from phyly_amd import engine as E
    _, opts, _, udk = _family(k, family)
    wl = ref.wl
    wl.setup_engine(eng)
    mask = (np.arange(wl.N) % 3 == 0).astype(np.int32)
    sel = mask.astype(bool)
    try:
        _set_options(eng, opts)
        for S, codes in ref.data.items():
            want = ref.marg[S]
            eng.set_patterns_codes(codes, wl.defs)
            wts = ref.weights(S)
            eng.set_site_weights(wts)
            got, sums = eng.marginal()
            assert eng.info(E.INFO_UPDOWN_KERNEL) == udk, S
            assert np.max(np.abs(got - want)) <= TOL, S
            ref_sum = _wsum(want, wts).astype(float)
            bound = SUM_TOL * _wsum(np.abs(want), np.abs(wts)).astype(float) + PROB_ULP * np.sum(np.abs(wts))
            assert np.all(np.abs((sums[..., 0] + sums[..., 1]) - ref_sum) <= bound), S
            _, fused = eng.marginal(per_site=False)                # summed as the up pass produces them
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
        eng.set_site_weights(None)
        _reset(eng)


@pytest.mark.parametrize("k,family", _cases())
def test_edge_expect(eng, ref, k, family):
    from phyly_amd import engine as E
    _, opts, _, udk = _family(k, family)
    wl = ref.wl
    wl.setup_engine(eng)
    sel = ref.xmask.astype(bool)
    try:
        _set_options(eng, opts)
        eng.set_patterns_codes(ref.data[ref.xS], wl.defs)
        eng.set_site_weights(None)
        for coef, mode in ((0, E.COEF_PRIOR), (1, E.COEF_PRIOR_RATE_EDGE)):
            want = ref.expect[coef]
            got, sums = eng.edge_expect(ref.L, mode, edge_mask=ref.xmask)
            assert eng.info(E.INFO_UPDOWN_KERNEL) == udk, mode
            assert _row_err(got[:, sel], want[:, sel]) <= TOL, mode
            assert np.all(got[:, ~sel] == 0.0), mode
            tot = (sums[:, 0] + sums[:, 1])[sel]
            bound = SUM_TOL * np.sum(np.max(np.abs(want[:, sel]), axis=1))
            assert np.max(np.abs(tot - want[:, sel].astype(np.longdouble).sum(axis=0).astype(float))) <= bound, mode
    finally:
        _reset(eng)


# ------------------------------------------------------------------ K1: transition and Frechet matrices
@pytest.mark.parametrize("k", [13, 14, 26, 27, 64])
def test_transition_matrices(eng, oracle, k):
    """the LDS form of the product (k <= 26) and the tiled global one (k >= 27), three categories (at odd k one of them
    the rate-0 category)"""
    wl = custom_workload(k, 3 if k == 64 else 6, C=3, invariable=0.2 if k % 2 else 0.0, root="custom", seed=5200 + k)
    wl.setup_engine(eng)
    P = eng.transition_matrices()
    m, ow = oracle_model(oracle, wl, wl.simulate(2))
    assert P.shape == ow["P"].shape == (3, wl.E, k, k)
    assert np.max(np.abs(P - ow["P"])) <= 4e-16
    np.testing.assert_allclose(P.sum(axis=-1), 1.0, rtol=0, atol=1e-14)


@pytest.mark.parametrize("k", [13, 14])
def test_frechet_matrices(eng, oracle, k):
    """the two forms of the Frechet block matrices (k < 14, k >= 14) against the binary128 ones"""
    from phyly_amd import engine as E
    wl = custom_workload(k, 6, C=3, invariable=0.2 if k % 2 else 0.0, root="none", seed=5300 + k)
    wl.setup_engine(eng)
    m, ow = oracle_model(oracle, wl, wl.simulate(2))
    L = np.random.default_rng(k).uniform(-1, 1, (k, k))
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
        assert np.max(np.abs(got - want) / np.maximum(scale, 1e-300)) <= 1e-14, coef


# ------------------------------------------------------------------ JSON level: the host layer at large k
def _json_query(rng, kind):
    """a feasible random query: positive edge rates, an irreducible Q, at least one positive category rate and no
    all-zero observation row, so that every site has a positive likelihood"""
    from test_gpu_differential import random_tree
    if kind in ("dwell", "trans"):
        k = rng.choice([9, 13, 17, 21, 27, 33, 48])                # one binary128 Frechet build per query in the oracle
    else:
        k = rng.choice(KS)
    n_nodes = rng.randrange(5, 9) if k >= 33 else rng.randrange(6, 12)
    edges = random_tree(rng, n_nodes)
    Q = nonreversible_rates(k, np.random.default_rng(rng.randrange(1 << 30)))
    Q[np.diag_indices(k)] = rng.choice([0.0, 5.0])                   # the diagonal is ignored
    md = {"edges": edges, "edge_rate_coefficients": [rng.uniform(0.01, 0.6) for _ in edges], "rate_matrix": Q.tolist()}
    nchar = k + 1 + rng.randrange(0, 3)
    defs = [[1.0 if j == c else 0.0 for j in range(k)] for c in range(k)] + [[1.0] * k]
    while len(defs) < nchar:
        defs.append([rng.choice([0, 0.5, 1]) for _ in range(k)])
        defs[-1][rng.randrange(k)] = 1.0
    S = rng.randrange(3, 40)
    md["character_definitions"] = defs
    md["character_data"] = [[rng.randrange(nchar) if rng.random() < 0.7 else k for _ in range(n_nodes)] for _ in range(S)]
    r = rng.random()
    if r < 0.4:
        md["rate_divisor"] = "equilibrium_exit_rate"
    elif r < 0.7:
        md["rate_divisor"] = rng.choice([0.5, 3.0, 40.0])
    r = rng.random()
    if r < 0.25:
        md["root_prior"] = "equilibrium_distribution"
    elif r < 0.5:
        md["root_prior"] = "uniform_distribution"
    elif r < 0.75:
        md["root_prior"] = [rng.uniform(0.01, 1.0) for _ in range(k)]
    ncat = 2 if k >= 48 else 3
    r = rng.random()
    if r < 0.3:
        md["gamma_rate_mixture"] = {"gamma_shape": rng.choice([0.5, 1.5]), "gamma_categories": ncat - 1,
                                    "invariable_prior": 0.2}
    elif r < 0.55:
        md["normalized_median_gamma_rate_mixture"] = {"gamma_shape": rng.choice([0.7, 2.0]), "gamma_categories": ncat}
    elif r < 0.8:
        rates = [rng.choice([0.0, 0.4, 1.0, 2.5]) for _ in range(ncat)]
        rates[0] = 1.0
        md["rate_mixture"] = {"rates": rates, "prior": "uniform_distribution" if rng.random() < 0.5 else
                              [x / sum(range(1, ncat + 1)) for x in range(1, ncat + 1)]}
    x = {"model_and_data": md}
    if kind in ("dwell", "trans"):
        x["edge_reduction"] = {"selection": [rng.randrange(len(edges)) for _ in range(2)]}
    if kind == "dwell":
        x["state_reduction"] = {"selection": [rng.randrange(k) for _ in range(3)],
                                "aggregation": [round(rng.uniform(-1, 2), 3) for _ in range(3)]}
    elif kind == "trans":
        pairs = [[rng.randrange(k), rng.randrange(k)] for _ in range(3)]
        x["trans_reduction"] = {"selection": pairs, "aggregation": rng.choice(["sum", [1.0, -0.5, 2.0]])}
    elif kind == "deriv" and rng.random() < 0.5:
        x["edge_reduction"] = {"selection": [rng.randrange(len(edges)) for _ in range(3)]}
    elif kind == "marginal" and rng.random() < 0.5:
        x["node_reduction"] = {"selection": [rng.randrange(n_nodes) for _ in range(3)]}
    if rng.random() < 0.5:
        x["site_reduction"] = {"aggregation": [round(rng.uniform(-2, 3), 3) for _ in range(S)]}
    return x


@pytest.mark.parametrize("kind", ["ll", "deriv", "marginal", "dwell", "trans"])
def test_json_queries_at_large_state_counts(oracle, kind):
    """compaction, character definitions, root prior, rate divisor and mixture forms mapped by the host layer for
    k up to 64, against the oracle's drivers; every query is feasible and is compared"""
    import arbplf
    from test_gpu_differential import _check
    from test_gpu_expect import _check_table
    prod = getattr(arbplf, "arbplf_" + kind)
    orc = getattr(oracle, "arbplf_" + kind)
    rng = random.Random({"ll": 71, "deriv": 72, "marginal": 73, "dwell": 74, "trans": 75}[kind])
    for _ in range(3):
        s = json.dumps(_json_query(rng, kind))
        want = json.loads(orc(s))
        assert all(np.isfinite(r[-1]) for r in want["data"])
        got = json.loads(prod(s))
        if kind in ("dwell", "trans"):
            _check_table(got, want)
        else:
            _check(kind, got, want)
