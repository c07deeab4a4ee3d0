"""GPU: plk_cat_posterior, plk_edge_pair_sums / plk_rate_matrix_sens and plk_mixture_sens against the oracle on the
asymmetric models of helpers.K4_MODELS, on helpers.QUERY_MODEL and on helpers.FAMILY_MODELS.

The tests these queries came with (test_gpu_cat_posterior, test_gpu_pair_sums, test_gpu_mixture_sens) run them on
synth.Workload models and on a 9- and a 5-taxon document: a reversible Q or the equilibrium root prior, stack need 1 - 2,
at most one unary and one three-way node, at most 6 character definitions.  Here: every root prior, the custom root
weights and OP_NODE_MUL of k_ll_fused4_catpost<4 | 8 | 16>, 7 and 17 definitions, a rate-0 edge on the tree of a rate-0
category with unequal priors, k_up4_pairsums / k_up4_mixsens after k_down_fused4<4>, <8> and k_down_store4, the second
pass of their fixed-grid batch loops, and the generic instantiations K = 2, 8, 16, 32, 64.
tests/test_query_family_models.py shows on the CPU that these models tell a wrong kernel from a right one.

Every engine is set up from the model's document with the rate divisor replaced by a number
(helpers.numeric_divisor_doc): mixsens_cases.expectations needs one, and the kernels do not care where Qn came from.
Site counts are 1, 65 and 257 (UD4_BLOCK = PS4_BLOCK = PLK_TILE = 256: one block and a partial wave), alternately simulated
and random with 10 % missing codes, each once without weights and once under test_gpu_pair_sums._weights (positive,
non-integer, about 15 % zeros).  Every case asserts the kernel it ran (PLK_INFO_CAT_POSTERIOR_KERNEL,
PLK_INFO_PAIR_SUMS_KERNEL, PLK_INFO_MIXTURE_SENS_KERNEL), PLK_INFO_STACK_SLOTS and, where the k = 4 up/down kernels ran,
PLK_INFO_DOWN4_KERNEL before its values.

Bars, unchanged from the tests named above: catpost_cases.rtol for posteriors and rates; 1e-12 of max|.| per
(category, edge) for W and per category for the root rows; 1e-11 of max|.| for G and its root row; 1e-12 of max_c |.|
for prior_out and rate_out (the rate of a rate-0 category: the rate_tol of mixsens_cases.expectations, at most 1e-8),
1e-13 for the three identities of plk_mixture_sens.

Oracle values (binary128) are built once per model; seconds on one CPU core for the three site counts together:
irregular 9, balanced32 2, balanced64 49, wide 2, balanced64g3 20 (W costs 16 C up/down passes per site and edge count);
the family models at 65 sites: k = 2: 1, 5: 1, 13: 12, 27: 36, 48: 67 (with the long-double W of FAMILY_LONG_DOUBLE; 67 and
95 with the binary128 one); the 241-taxon model of the k_down_store4 test (C = 1, 33 sites): 1.  The oracle runs its sites
on every core it is given."""
import subprocess
import sys

import numpy as np
import pytest

import catpost_cases
import mixsens_cases
import qgrad_cases
from helpers import K4_MODELS, QUERY_MODEL, deep_workload, family_workload, numeric_divisor_doc, query_workload, tree_workload
from phyly_amd import engine as E_, synth
from test_gpu_pair_sums import _check, _weights

pytestmark = pytest.mark.gpu
LD = np.longdouble

MODELS = K4_MODELS + (QUERY_MODEL,)
# stack need, categories, character definitions (tests/test_gpu_k4_variants.py: SHAPE) and the down pass run_updown4
# prescribes: k_down_fused4<D> with D = 4 for at most 4 slots, 8 for at most 8 (every model stages fewer than 240 rows)
SHAPE = {"irregular": dict(slots=1, C=4, nchar=7, down=4), "balanced32": dict(slots=4, C=1, nchar=5, down=4),
         "balanced64": dict(slots=5, C=5, nchar=5, down=8), "wide": dict(slots=1, C=2, nchar=17, down=4),
         QUERY_MODEL: dict(slots=5, C=3, nchar=5, down=8)}
SIZES = (1, 65, 257)
GS = 65                              # rate_matrix_sens: irregular and QUERY_MODEL
SENS_MODELS = ("irregular", QUERY_MODEL)
FAMILY_KS = (2, 5, 13, 27, 48)       # K = 2, 8, 16, 32, 64
# the binary128 W of 65 sites costs 44 s at k = 27 and 71 s at k = 48 (2k + 1 up/down passes per category and site;
# the long-double one about half), so
# there the 65 sites are compared with the oracle's long-double W (precise = 1), which _Ref first holds against the
# binary128 one on the first 5 sites to 1e-14 of the largest entry: two decades inside the 1e-12 bar, which stays
# (the precedent: HESS_LONG_DOUBLE of tests/test_gpu_k4_variants.py)
FAMILY_LONG_DOUBLE = (27, 48)

def _ld(x):
    return np.asarray(x[..., 0], dtype=LD) + np.asarray(x[..., 1], dtype=LD)


def _wsum(vals, wt):
    return np.tensordot(np.asarray(wt, dtype=LD), np.asarray(vals, dtype=LD), axes=(0, 0))


def _site_weights(S):
    """(None, weights): no weights once, then test_gpu_pair_sums._weights; a lone site keeps a positive weight"""
    wt = _weights(S, 900 + S)
    if wt[0] == 0.0:
        wt[0] = 0.7
    return (None, wt)


def _dense_doc(md):
    out = {key: v for key, v in md.items() if key not in ("character_definitions", "character_data")}
    out["probability_array"] = np.asarray(md["character_definitions"], dtype=float)[np.asarray(md["character_data"])].tolist()
    return out


_DEFAULTS = {E_.OPT_FORCE_GENERIC: 0, E_.OPT_SITE_CHUNK: 0}


def _reset(eng):
    eng.set_site_weights(None)
    for o, v in _DEFAULTS.items():
        eng.set_option(o, v)


@pytest.fixture(scope="module")
def eng():
    from phyly_amd.engine import Engine
    e = Engine(0)
    yield e
    _reset(e)
    e.close()


class _Ref:
    """oracle values of one workload at the given site counts, built once: posteriors, per-site W and root rows (summed
    under each weight vector by the tests), the mixture sums under each weight vector"""

    def __init__(self, oracle, wl, sizes, factored=False, sens=False, long_double=False):
        self.wl = wl
        self.data = {S: (wl.simulate(S) if i % 2 == 0 else wl.random_codes(S, seed=S, missing_frac=0.1)) for i, S in enumerate(sizes)}
        self.doc, self.m, self.post, self.W, self.R, self.mix, self.mix_cache = {}, {}, {}, {}, {}, {}, {}
        for S, codes in self.data.items():
            md = self.doc[S] = numeric_divisor_doc(wl, codes)
            m = self.m[S] = oracle.parse_model(md)
            self.w = w = oracle.prepare(m)
            self.post[S] = (m, w) + catpost_cases.posteriors(oracle, m, w, precise=2, B=m.B)
            if long_double:
                self.W[S] = qgrad_cases.oracle_W_factored(oracle, m, w, None, precise=1)
                exact = qgrad_cases.oracle_W_factored(oracle, m, w, None, sites=slice(0, 5))
                assert np.max(np.abs(self.W[S][:5] - exact)) <= 1e-14 * np.max(np.abs(exact))
            else:
                self.W[S] = (qgrad_cases.oracle_W_factored if factored else qgrad_cases.oracle_W)(oracle, m, w, None)
            self.R[S] = qgrad_cases.oracle_root(oracle, m, w, None, per_category=True)
            self.mix_cache[S] = {}
            for wt in _site_weights(S):
                self.mix[S, wt is not None] = mixsens_cases.expectations(oracle, md, np.ones(S) if wt is None else wt, cache=self.mix_cache[S])
        self.k0 = mixsens_cases.product_k0(m)
        if sens:
            self.G = qgrad_cases.oracle_G(oracle, self.m[GS], self.w, _site_weights(GS)[1])


_REFS = {}


@pytest.fixture
def ref(oracle, request):
    model = request.node.callspec.params["model"]
    if model not in _REFS:
        _REFS[model] = _Ref(oracle, query_workload(model), SIZES, sens=model in SENS_MODELS)
    return _REFS[model]


def _check_shape(eng, model):
    s = SHAPE[model]
    assert eng.info(E_.INFO_STACK_SLOTS) == s["slots"] and eng.info(E_.INFO_CATEGORIES) == s["C"]


def _check_mixture(tag, po, ro, want):
    """prior_out and rate_out against mixsens_cases.expectations: 1e-12 of max_c |.|, the rate of a rate-0 category its
    rate_tol"""
    want_p, want_r, tol_r = want
    assert np.all(np.isfinite(po)) and np.all(np.isfinite(ro))
    ep = np.abs(_ld(po) - want_p) / np.max(np.abs(want_p))
    er = np.abs(_ld(ro) - want_r) / np.max(np.abs(want_r))
    print("%s: prior_out %.3g, rate_out %.3g of max|.| (bound 1e-12; rate-0 categories %.3g)" % (tag, float(np.max(ep)), float(np.max(np.where(tol_r == 0, er, 0))), float(np.max(tol_r))))
    assert np.all(ep <= 1e-12), tag
    assert np.all(er <= np.maximum(tol_r, LD(1e-12))), tag


def _check_identities(tag, eng, k0, m, wt, po, ro):
    """test_gpu_mixture_sens.test_identities: sum_c p_c prior_out[c] = sum_s w_s; sum_c r_c rate_out[c] = sum_e t_e
    (plk_deriv edge sums); p_c prior_out[c] = post_sums[c] of plk_cat_posterior -- all to 1e-13"""
    p, rate = np.asarray(k0["cat_prior"], dtype=LD), np.asarray(k0["cat_rates"], dtype=LD)
    got_p, got_r = _ld(po), _ld(ro)
    _, dsum = eng.deriv(per_site=False)
    _, _, psum, _ = eng.cat_posterior(per_site=False)
    sw = np.sum(np.asarray(wt, dtype=LD))
    e1 = float(abs(np.sum(p * got_p) - sw) / sw)
    rhs = np.sum(np.asarray(m.edge_rates_csr, dtype=LD) * _ld(dsum))
    scale = max(np.max(np.abs(rate * got_r)), abs(rhs))        # the terms cancel: relative to the largest of them
    e2 = float(abs(np.sum(rate * got_r) - rhs) / scale)
    e3 = float(np.max(np.abs(p * got_p - _ld(psum))) / sw)
    print("%s: identities %.3g %.3g %.3g (bound 1e-13)" % (tag, e1, e2, e3))
    assert e1 <= 1e-13 and e2 <= 1e-13 and e3 <= 1e-13, tag


# ------------------------------------------------------------------ the k = 4 models
def _cases(model, limit):
    """-> [(name, options, dense, kernel)]: kernel 1 for compact codes and at most `limit` categories, else 2"""
    k4 = 1 if SHAPE[model]["C"] <= limit else 2
    return [("codes", {}, False, k4), ("generic", {E_.OPT_FORCE_GENERIC: 1}, False, 2), ("dense", {}, True, 2)]


def _params(limit):
    return [pytest.param(mdl, c[0], id="%s-%s" % (mdl, c[0])) for mdl in MODELS for c in _cases(mdl, limit)]


def _setup(eng, oracle, ref, S, opts, dense):
    for o, v in opts.items():
        eng.set_option(o, v)
    md = ref.doc[S]
    mixsens_cases.setup_engine(eng, oracle, _dense_doc(md) if dense else md)


@pytest.mark.parametrize("model,case", _params(8))
def test_cat_posterior(eng, oracle, ref, model, case):
    """k_ll_fused4_catpost<4> (slots <= 4) and <8> (the balanced64 trees) under every root prior, with OP_NODE_MUL
    (irregular, wide) and 8-bit staged codes (wide); the generic kernel forced and on the dense layout"""
    _, opts, dense, kernel = next(c for c in _cases(model, 8) if c[0] == case)
    wl = ref.wl
    assert wl.defs.shape == (SHAPE[model]["nchar"], 4)
    try:
        for S in ref.data:
            _setup(eng, oracle, ref, S, opts, dense)
            codes = ref.data[S]
            assert SHAPE[model]["nchar"] <= 16 or S < 65 or np.sum(codes >= 16) >= 10, S
            catpost_cases.check_engine(eng, oracle, wl, codes, "%s %s S=%d" % (model, case, S), kernel, ref=ref.post[S],
                                       site_weights=_site_weights(S)[1])
            _check_shape(eng, model)
    finally:
        _reset(eng)


@pytest.mark.parametrize("model,case", _params(4))
def test_edge_pair_sums(eng, oracle, ref, model, case):
    """k_up4_pairsums after k_down_fused4<4 | 8> (balanced64 with C = 5: the generic kernel), with and without an edge
    mask; plk_rate_matrix_sens on irregular and helpers.QUERY_MODEL"""
    _, opts, dense, kernel = next(c for c in _cases(model, 4) if c[0] == case)
    E = ref.wl.E
    mask = np.array([(e * 7 + 3) % 3 != 0 for e in range(E)], dtype=np.int32)
    try:
        for S in ref.data:
            _setup(eng, oracle, ref, S, opts, dense)
            for wt in _site_weights(S):
                tag = "%s %s S=%d weighted=%s" % (model, case, S, wt is not None)
                eng.set_site_weights(wt)
                W, R = eng.edge_pair_sums()
                assert eng.info(E_.INFO_PAIR_SUMS_KERNEL) == kernel, tag
                _check_shape(eng, model)
                if kernel == 1:
                    assert eng.info(E_.INFO_DOWN4_KERNEL) == SHAPE[model]["down"], tag
                ws = np.ones(S) if wt is None else wt
                _check(tag + " W", _ld(W), _wsum(ref.W[S], ws), 1e-12)
                _check(tag + " root", _ld(R), _wsum(ref.R[S], ws), 1e-12)
                Wm, _ = eng.edge_pair_sums(edge_mask=mask)
                assert eng.info(E_.INFO_PAIR_SUMS_KERNEL) == kernel, tag
                assert np.any(mask == 0) and np.all(Wm[:, mask == 0] == 0), tag
                assert np.array_equal(Wm[:, mask != 0], W[:, mask != 0]), tag
                if model in SENS_MODELS and S == GS and wt is not None:
                    G, root = eng.rate_matrix_sens()
                    assert eng.info(E_.INFO_PAIR_SUMS_KERNEL) == kernel, tag
                    want_root = np.sum(_wsum(ref.R[S], ws), axis=0)
                    eg = float(np.max(np.abs(_ld(G) - ref.G)) / np.max(np.abs(ref.G)))
                    er = float(np.max(np.abs(_ld(root) - want_root)) / np.max(np.abs(want_root)))
                    print("%s: G %.3g of max|G|, root %.3g of max|root| (bound 1e-11)" % (tag, eg, er))
                    assert eg <= 1e-11 and er <= 1e-11, tag
    finally:
        _reset(eng)


@pytest.mark.parametrize("model,case", _params(4))
def test_mixture_sens(eng, oracle, ref, model, case):
    """k_up4_mixsens after k_down_fused4<4 | 8>; the generic kernel forced, on the dense layout and for C = 5"""
    _, opts, dense, kernel = next(c for c in _cases(model, 4) if c[0] == case)
    try:
        for S in ref.data:
            _setup(eng, oracle, ref, S, opts, dense)
            for wt in _site_weights(S):
                tag = "%s %s S=%d weighted=%s" % (model, case, S, wt is not None)
                eng.set_site_weights(wt)
                po, ro = eng.mixture_sens()
                assert eng.info(E_.INFO_MIXTURE_SENS_KERNEL) == kernel, tag
                _check_shape(eng, model)
                if kernel == 1:
                    assert eng.info(E_.INFO_DOWN4_KERNEL) == SHAPE[model]["down"], tag
                _check_mixture(tag, po, ro, ref.mix[S, wt is not None])
                _check_identities(tag, eng, ref.k0, ref.m[S], np.ones(S) if wt is None else wt, po, ro)
    finally:
        _reset(eng)


# ------------------------------------------------------------------ k_down_store4
STORE_T, STORE_S = 241, 33


def _store_workload():
    """241 taxa on a Yule tree, one rate category, no root prior: 241 staged code rows of 256 bytes are 61 696 bytes"""
    shell = synth.Workload(T=STORE_T, k=4, tree="yule", model="hky85", seed=4241)
    return tree_workload(4, shell.edges, shell.edge_rates, root="none", seed=4241, name="k4 241 taxa")


def test_down_store4(eng, oracle):
    """k_down_store4 is the down pass when the staged code rows of the observed nodes do not fit the 60 KiB
    run_updown4 allows k_down_fused4 (nobs * 256 bytes: more than 240 observed nodes) or when the tree needs more than
    16 slots (at least 2^17 leaves).  The smallest input is the first: 241 leaves, no data on internal nodes.  The
    pair-sum, mixture-gradient and derivative passes on it, against the oracle."""
    wl = _store_workload()
    assert wl.T == STORE_T and 256 * (STORE_T - 1) <= 60 * 1024 < 256 * STORE_T
    r = _Ref(oracle, wl, (STORE_S,))
    S = STORE_S
    try:
        mixsens_cases.setup_engine(eng, oracle, r.doc[S])
        for wt in _site_weights(S):
            tag = "241 taxa weighted=%s" % (wt is not None)
            ws = np.ones(S) if wt is None else wt
            eng.set_site_weights(wt)
            W, R = eng.edge_pair_sums()
            assert eng.info(E_.INFO_PAIR_SUMS_KERNEL) == 1 and eng.info(E_.INFO_DOWN4_KERNEL) == 0, tag
            assert eng.info(E_.INFO_STACK_SLOTS) <= 16
            _check(tag + " W", _ld(W), _wsum(r.W[S], ws), 1e-12)
            _check(tag + " root", _ld(R), _wsum(r.R[S], ws), 1e-12)
            po, ro = eng.mixture_sens()
            assert eng.info(E_.INFO_MIXTURE_SENS_KERNEL) == 1 and eng.info(E_.INFO_DOWN4_KERNEL) == 0, tag
            _check_mixture(tag, po, ro, r.mix[S, wt is not None])
            _check_identities(tag, eng, r.k0, r.m[S], ws, po, ro)
            assert eng.info(E_.INFO_UPDOWN_KERNEL) == 1 and eng.info(E_.INFO_DOWN4_KERNEL) == 0, tag      # the plk_deriv of the identities
    finally:
        _reset(eng)


# ------------------------------------------------------------------ the 16-slot instantiations
def test_sixteen_slots(eng, oracle):
    """k_ll_fused4_catpost<16> and the pair-sum and mixture-gradient passes on helpers.deep_workload (stack need 9) with
    a two-category mixture of unequal priors, 257 all-missing sites (the only data its LDS image admits, see
    test_gpu_k4_variants.test_ll_sixteen_slot_interpreter).  Expected values are analytic: every partial vector is 1, so
    post[s][c] = prior_c, rate = sum_c prior_c r_c, prior_out[c] = sum_s w_s, rate_out[c] = 0 and
    <W[c][e], P[c][e]> = prior_c sum_s w_s on every edge (P from the oracle's prepared model).  run_updown4 gives this tree
    k_down_store4: its 512 staged leaf rows are 128 KiB, beyond the 60 KiB of k_down_fused4, and no tree of stack need
    9 to 16 has fewer than 241 observed nodes, so k_down_fused4<16> is out of reach of any input.
    Such data cannot tell a wrong traversal from a right one; this pins dispatch, launch and scaling.

    Bars: catpost_cases.rtol; prior_out 1e-12 of max_c; <W, P> sums 16 entries of W held to 1e-12 of max|W[c][e]| with
    weights P that add up to 4: 4e-12 of max|W[c][e]|; rate_out[c] is a sum of terms prior_c w_s t_e fe^T Qn P 1 / L whose
    positive and negative parts are each at most prior_c w_s t_e max|Qn_ii|: 1e-12 of prior_c sum_s w_s sum_e t_e max|Qn_ii|."""
    from helpers import oracle_model
    rates, prior = np.array([0.3, 1.7]), np.array([0.35, 0.65])
    wl = deep_workload(rate_mixture=dict(rates=rates.tolist(), prior=prior.tolist()))
    S = 257
    codes = np.zeros((wl.N, S), dtype=np.uint8)
    m, w = oracle_model(oracle, wl, codes)
    k0 = wl.prepare()
    assert np.array_equal(k0["cat_prior"], w["cat_prior"]) and np.max(np.abs(k0["cat_rates"] - w["cat_rates"])) <= 1e-15
    cp, cr = np.asarray(w["cat_prior"], dtype=LD), np.asarray(w["cat_rates"], dtype=LD)
    wl.setup_engine(eng)
    try:
        eng.set_patterns_codes(codes, wl.defs)
        want_post = np.broadcast_to(cp, (S, 2))
        want_rate = np.full(S, np.sum(cp * cr))
        tol = catpost_cases.rtol(wl.E, 4, 2)
        for wt in _site_weights(S):
            tag = "deep weighted=%s" % (wt is not None)
            sw = LD(S) if wt is None else np.sum(wt.astype(LD))
            eng.set_site_weights(wt)
            gp, gr, psum, rsum = eng.cat_posterior()
            assert eng.info(E_.INFO_CAT_POSTERIOR_KERNEL) == 1 and eng.info(E_.INFO_STACK_SLOTS) == 9, tag
            catpost_cases.compare(tag, gp, gr, want_post, want_rate, tol)
            assert np.all(np.abs(_ld(psum) - cp * sw) <= tol * cp * sw), tag
            W, R = eng.edge_pair_sums()
            assert eng.info(E_.INFO_PAIR_SUMS_KERNEL) == 1 and eng.info(E_.INFO_DOWN4_KERNEL) == 0, tag
            Wl = _ld(W)
            dot = np.einsum("ceij,ceij->ce", Wl, np.asarray(w["P"], dtype=LD))
            err = np.abs(dot - (cp * sw)[:, None]) / np.max(np.abs(Wl), axis=(2, 3))
            print("%s: <W, P> vs prior_c sum w: %.3g of max|W[c][e]| (bound 4e-12)" % (tag, float(np.max(err))))
            assert np.all(np.isfinite(W)) and np.all(err <= 4e-12), tag
            po, ro = eng.mixture_sens()
            assert eng.info(E_.INFO_MIXTURE_SENS_KERNEL) == 1 and eng.info(E_.INFO_DOWN4_KERNEL) == 0, tag
            assert np.all(np.abs(_ld(po) - sw) <= 1e-12 * sw), tag
            scale = cp * sw * np.sum(np.asarray(m.edge_rates_csr, dtype=LD)) * np.max(np.abs(np.diag(w["Qn"])))
            print("%s: rate_out %s of its terms (bound 1e-12)" % (tag, np.asarray(np.abs(_ld(ro)) / scale, dtype=float)))
            assert np.all(np.abs(_ld(ro)) <= 1e-12 * scale), tag
    finally:
        _reset(eng)


# ------------------------------------------------------------------ the second pass of the fixed-grid batch loops
_CUS = []


def _compute_units():
    """torch's multi_processor_count of device 0, asked once in a child process (as the other tests ask torch: in this
    process, beside the engine, torch finds no device)"""
    if not _CUS:
        r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode == 0, r.stderr.decode()[-400:]
        _CUS.append(int(r.stdout.decode().split()[-1]))
    return _CUS[0]


def _second_pass(eng, oracle, ref, block, force_generic):
    """S = 4 CUs * block + 257 (or 65) sites of `irregular`: one batch more than 4 CUs workgroups, so workgroups 0 .. make a
    second pass of `for (bt = blockIdx.x; bt < nbatch; bt += gridDim.x)`.  The alignment tiles the oracle's patterns,
    site s showing pattern s mod P; 4 CUs * block is no multiple of P, so every lane meets another pattern on its second
    pass than on its first.  Weights are drawn per site; the reference is the oracle's per-pattern value under the
    long-double sum of the weights of the pattern's sites: exact aggregation.  Bars as in the tests above.
    Device memory (per_site of run_updown4 / run_updown): 377 doubles per site for the k = 4 kernels (0.8 GB at
    256 CUs), 1161 for the generic ones (0.6 GB at a quarter of the sites)."""
    cus = _compute_units()
    P = 257 if block == 256 else 65
    S = 4 * cus * block + P
    nbatch = (S + block - 1) // block
    assert nbatch > 4 * cus
    pat = np.arange(S) % P
    lanes = np.arange(4 * cus * block, S)
    assert np.all(pat[lanes] != pat[lanes - 4 * cus * block])
    codes = np.ascontiguousarray(ref.data[P][:, pat])
    wt = _weights(S, 77)
    agg = np.zeros(P, dtype=LD)
    np.add.at(agg, pat, wt.astype(LD))
    m = ref.m[P]
    want_mix = mixsens_cases.expectations(oracle, ref.doc[P], agg, cache=ref.mix_cache[P])
    kernel = 2 if force_generic else 1
    try:
        eng.set_option(E_.OPT_FORCE_GENERIC, force_generic)
        mixsens_cases.setup_engine(eng, oracle, ref.doc[P], S=1)
        eng.set_patterns_codes(codes, ref.wl.defs)
        eng.set_site_weights(wt)
        tag = "irregular S=%d kernel %d" % (S, kernel)
        W, R = eng.edge_pair_sums()
        assert eng.info(E_.INFO_PAIR_SUMS_KERNEL) == kernel and eng.info(E_.INFO_STACK_SLOTS) == 1, tag
        if kernel == 1:
            assert eng.info(E_.INFO_DOWN4_KERNEL) == 4, tag
        _check(tag + " W", _ld(W), _wsum(ref.W[P], agg), 1e-12)
        _check(tag + " root", _ld(R), _wsum(ref.R[P], agg), 1e-12)
        po, ro = eng.mixture_sens()
        assert eng.info(E_.INFO_MIXTURE_SENS_KERNEL) == kernel, tag
        if kernel == 1:
            assert eng.info(E_.INFO_DOWN4_KERNEL) == 4, tag
        _check_mixture(tag, po, ro, want_mix)
        _check_identities(tag, eng, ref.k0, m, wt, po, ro)
    finally:
        _reset(eng)


@pytest.mark.parametrize("model", ["irregular"])
def test_second_pass_k4(eng, oracle, ref, model):
    """k_up4_pairsums and k_up4_mixsens (PS4_BLOCK = 256): the lane that stored F_b for a site reads it back"""
    _second_pass(eng, oracle, ref, 256, 0)


@pytest.mark.parametrize("model", ["irregular"])
def test_second_pass_generic(eng, oracle, ref, model):
    """k_up_pairsums<4> and k_up_mixsens<4> (GEN_BLOCK = 64), forced generic on the same model"""
    _second_pass(eng, oracle, ref, 64, 1)


# ------------------------------------------------------------------ the generic instantiations
@pytest.mark.parametrize("k", FAMILY_KS)
def test_generic_instantiations(eng, oracle, k):
    """k_catpost_generic<K>, k_up_pairsums<K> and k_up_mixsens<K> for K = 2, 8, 16, 32, 64 on helpers.FAMILY_MODELS
    (k = 2, 5, 13, 27, 48: root priors none and custom, data on internal nodes, rate-0 categories, C = 2 .. 4), 65 sites;
    W from qgrad_cases.oracle_W_factored"""
    wl = family_workload(k)
    S = 65
    r = _Ref(oracle, wl, (S,), factored=True, long_double=k in FAMILY_LONG_DOUBLE)
    C = int(r.w["C"])
    try:
        mixsens_cases.setup_engine(eng, oracle, r.doc[S])
        assert eng.k == k and eng.info(E_.INFO_CATEGORIES) == C
        catpost_cases.check_engine(eng, oracle, wl, r.data[S], "k=%d" % k, 2, ref=r.post[S], site_weights=_site_weights(S)[1])
        for wt in _site_weights(S):
            tag = "k=%d C=%d weighted=%s" % (k, C, wt is not None)
            ws = np.ones(S) if wt is None else wt
            eng.set_site_weights(wt)
            W, R = eng.edge_pair_sums()
            assert eng.info(E_.INFO_PAIR_SUMS_KERNEL) == 2 and eng.k == k, tag
            _check(tag + " W", _ld(W), _wsum(r.W[S], ws), 1e-12)
            _check(tag + " root", _ld(R), _wsum(r.R[S], ws), 1e-12)
            po, ro = eng.mixture_sens()
            assert eng.info(E_.INFO_MIXTURE_SENS_KERNEL) == 2, tag
            _check_mixture(tag, po, ro, r.mix[S, wt is not None])
            _check_identities(tag, eng, r.k0, r.m[S], ws, po, ro)
    finally:
        _reset(eng)
