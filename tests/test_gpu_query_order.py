"""GPU: on an engine that has seen any history, every query returns bit for bit what the same query returns on a fresh
engine that was brought to the same state and ran nothing else.

The engine decides what to recompute from six flags (prog_dirty, fmt_dirty, tables_dirty, model_dirty, dp_valid,
cp_kind / cp_tables_valid) and keeps a dozen grow-only device buffers; ten queries read that state, nine calls change it.
A wrong flag gives a stale table or a stale dP: wrong numbers and no fault.

One case per (family, change).  A family is a workload on one kernel family (FAMILIES; the case first asserts with
PLK_INFO_* that the family runs what its name says); a change toggles the engine between two states A and B (CHANGES).
The walk (tests/query_order_cases.py; its coverage claim is checked on the CPU by tests/test_query_order_walk.py) is a
cyclic order of the ten QUERIES in which every ordered pair, a query after itself included, stands as neighbours once.
test_query_order runs it on ONE live engine with the change applied between every two consecutive queries, once starting
in A, once starting in B: every (q1, q2) is seen as "q1 at A, change, q2 at B" and as "q1 at B, change, q2 at A", 200
triples.  There the second query of a pair always finds the engine freshly changed, never what the first one left half
done, so test_query_pairs_after_one_change runs the same order on another live engine with the change before every second
query only: every (q1, q2) once as "change, q1, q2" (the two tests share the fresh answers of a case).
Every answer is compared (np.array_equal on every array, == on every {hi, lo} pair) with the cached answer of a fresh
engine: a new engine per (state, query), set up for that state by set_option / set_tree / set_model / set_patterns /
set_site_weights alone, which runs that one query and is closed.  The PLK_INFO_* kernel values the query leaves are
compared too, so a wrong kernel choice that happens to give the right numbers is seen.

Bit equality compares the product with itself, so the fresh answers of ll, masked deriv, summed marginal and
cat_posterior are also held to the oracle at both states of every case, at the bars of the tests of those queries
(TOL, SUM_TOL, PROB_ULP, _row_err of tests/test_gpu_kernel_families.py; catpost_cases.rtol and compare).  As in
tests/test_gpu_updown_drivers.py the sites show P = 7 patterns, site s pattern s mod 7 (7 is coprime to every block and
chunk size), so the oracle (binary128) runs on 7 sites and the sums are its per-pattern values under the summed weights
of each pattern, in long double.  Prepared oracle workspaces and per-pattern values are cached at module scope.

No query is exempt from bit equality."""
import copy
import ctypes

import numpy as np
import pytest

import catpost_cases
from helpers import family_workload, query_workload, rel_err, tree_workload
from phyly_amd import engine as E_, synth
from query_order_cases import held_walk, walk
from test_gpu_k4_stream import _workload as _k4_workload, caterpillar
from test_gpu_kernel_families import PROB_ULP, SUM_TOL, TOL, _row_err
from test_gpu_polytomy import GAMMA4, _ordinary, star

pytestmark = pytest.mark.gpu
LD = np.longdouble

QUERIES = ("ll", "deriv", "marginal_sums", "marginal", "expect", "cat_posterior", "pair_sums", "rate_matrix_sens",
           "mixture_sens", "second_order")
# the queries that leave nothing of the shared preparation undone: they make, or have K1 make, dP (query_order_cases.held_walk)
FULL = ("deriv", "marginal_sums", "marginal", "second_order")
GROUNDED = ("ll", "deriv", "marginal_sums", "cat_posterior")
P = 7
FUSED4, GENERIC, MFMA, VEC, HESS4 = 1, 2, 3, 4, 5

# family -> (S_A, S_B)
FAMILIES = {"k4-stream": (300, 129), "k4-deep": (257, 130), "k4-star": (130, 130), "k20": (257, 130), "k61": (130, 70)}
# The "options" change puts every query on its generic kernel under 64-site chunks, where one second-order query is E + 1
# passes per chunk (0.95 s on k4-deep at S = 257, 0.67 s on k4-star at 130; twelve of them in a case).  Those three cases
# run both states at 70 sites (one full chunk and one of 6 sites), which keeps them under 10 s with every pair in place.
OPTIONS_S = {"k4-deep": 70, "k4-star": 70, "k61": 70}
CHANGES = ("none", "touch", "rates", "mixture", "root", "weights", "patterns", "layout", "options", "tree", "fit", "refused")
ONLY = {"layout": ("k4-stream", "k20"), "tree": ("k4-stream", "k20")}
CASES = [(f, c) for f in FAMILIES for c in CHANGES if f in ONLY.get(c, FAMILIES)]


# ------------------------------------------------------------------------------------------------ workloads and states
def _base_workload(family):
    if family == "k4-stream":
        return _k4_workload(caterpillar(8), seed=51)                       # gamma 4, equilibrium root prior, nchar = 5
    if family == "k4-deep":
        return query_workload("balanced64g3")
    if family == "k4-star":
        return tree_workload(4, star(40), _ordinary(40, 40), root="equilibrium", seed=9040, gamma=GAMMA4, nchar=5, name="star40")
    return family_workload(20 if family == "k20" else 61)


def _variant(wl, **kw):
    """a copy of the workload with some attributes replaced; K0 and the simulator tables are made anew"""
    v = copy.copy(wl)
    v.k0 = v._cum = None
    for name, val in kw.items():
        setattr(v, name, val)
    if "edge_rates_csr" in kw:
        v.edge_rates = [float(v.edge_rates_csr[pos]) for pos in v.order]
    return v


def _other_topology(wl):
    """the same taxa on another topology: leaf i takes the place of leaf T - 1 - i (leaves are nodes 0 .. T - 1)"""
    leaf = np.flatnonzero(wl.indptr[1:] == wl.indptr[:-1])
    T = len(leaf)
    assert np.array_equal(leaf, np.arange(T))
    edges = [[a, T - 1 - b if b < T else b] for a, b in wl.edges]
    indptr, indices, preorder, order = synth.csr_from_edges(edges)
    v = _variant(wl, edges=edges, indptr=indptr, indices=indices, preorder=preorder, order=order)
    rates = np.zeros(wl.E)
    rates[order] = wl.edge_rates
    v.edge_rates_csr = rates
    assert not np.array_equal(v.indices, wl.indices)
    return v


def _patterns(wl, seed):
    """codes[N][P]: simulated sites, then random ones with missing data; with definitions past the all-ones row, two
    leaves show one each whatever the draw gave"""
    pats = np.concatenate([wl.simulate(P - 2), wl.random_codes(2, seed=seed, missing_frac=0.1)], axis=1)
    if wl.nchar > wl.k + 1:
        pats[0, 0], pats[1, 1] = wl.nchar - 1, wl.k + 1
    return np.ascontiguousarray(pats, dtype=np.uint8)


def _weights(S):
    w = np.random.default_rng(S).uniform(0.25, 4.0, S)
    w[::5] = 0.0
    return w


class State:
    """what a fresh engine is brought to: options, tree, model (rates, mixture, root prior), patterns, weights"""

    def __init__(self, family, wl, wl_tag, pats, pats_tag, S, weights=None, dense=False, options=(0, 0), update_from=None):
        self.family, self.wl, self.wl_tag, self.pats, self.pats_tag, self.S = family, wl, wl_tag, pats, pats_tag, S
        self.weights, self.dense, self.options, self.update_from = weights, dense, options, update_from
        self.site_pat = np.arange(S) % P
        self.codes = np.ascontiguousarray(pats[:, self.site_pat])
        self.emask = np.array([(e * 5 + 1) % 3 != 0 for e in range(wl.E)], dtype=np.int32)
        self.nmask = (np.arange(wl.N) % 3 != 1).astype(np.int32)
        k0 = wl.prepare()
        self.C = int(k0["C"])
        off = ~np.eye(wl.k, dtype=bool)
        # em-update's pair: the rate-weighted dwell (minus the diagonal of Qn) and the transitions (its off-diagonal part)
        self.Ls = np.stack([np.where(off, 0.0, -k0["Qn"]), np.where(off, k0["Qn"], 0.0)])
        self.Ls_lo = np.stack([np.where(off, 0.0, -k0["Qn_lo"]), np.where(off, k0["Qn_lo"], 0.0)])

    def but(self, **kw):
        args = dict(family=self.family, wl=self.wl, wl_tag=self.wl_tag, pats=self.pats, pats_tag=self.pats_tag, S=self.S,
                    weights=self.weights, dense=self.dense, options=self.options, update_from=self.update_from)
        args.update(kw)
        return State(**args)

    def set_options(self, eng):
        eng.set_option(E_.OPT_SITE_CHUNK, self.options[0])
        eng.set_option(E_.OPT_FORCE_GENERIC, self.options[1])

    def set_model(self, eng, rates=None):
        k0 = self.wl.prepare()
        mode, rw = self.wl.root_engine()
        eng.set_model(k0["Qn"], self.wl.edge_rates_csr if rates is None else rates, k0["cat_rates"], k0["cat_prior"], mode, rw,
                      Qn_lo=k0["Qn_lo"])

    def set_patterns(self, eng):
        """the upload alone where the state has no weights: new patterns drop the weights of the old ones"""
        if self.dense:
            eng.set_patterns_dense(np.ascontiguousarray(self.wl.defs[self.codes.T].transpose(1, 2, 0)))
        else:
            eng.set_patterns_codes(self.codes, self.wl.defs)
        if self.weights is not None:
            eng.set_site_weights(self.weights)

    def bring(self, eng):
        self.set_options(eng)
        eng.set_tree(self.wl.indptr, self.wl.indices, self.wl.preorder)
        self.set_model(eng, self.update_from)
        if self.update_from is not None:
            eng.update_edge_rates(self.wl.edge_rates_csr)
        self.set_patterns(eng)


def _mixtures(family, wl):
    """(mixture of A, mixture of B): k = 4: C = 5 (gamma 4 + invariable) and C = 3, across the C <= 4 kernels; k = 20 / 61:
    the family's C and C - 1"""
    if wl.k == 4:
        return dict(gamma_shape=0.7, gamma_categories=4, invariable_prior=0.1), dict(gamma_shape=0.7, gamma_categories=3)
    b = dict(wl.mixture, gamma_categories=wl.mixture["gamma_categories"] - 1)
    return dict(wl.mixture), (b if b["gamma_categories"] > 1 or "invariable_prior" in b else None)


def _zero_rate_edge(wl, pats):
    """a CSR edge to a leaf whose parent shows the all-ones row at every pattern: rate 0 there leaves every site a
    positive likelihood"""
    for a in range(wl.N):
        if np.all(pats[a] == wl.k):
            for e in range(wl.indptr[a], wl.indptr[a + 1]):
                b = wl.indices[e]
                if wl.indptr[b + 1] == wl.indptr[b]:
                    return e
    raise AssertionError("no such edge")


def _fit_rates(A):
    e = E_.Engine(0)
    try:
        A.bring(e)
        return e.fit_edge_rates(A.wl.edge_rates_csr, E_.FIT_EM, max_iter=2, ftol=0.0)[0]
    finally:
        e.close()


def _states(family, change):
    """-> (A, B, move, the family's own state); move(live, src, dst, n) takes the live engine from src to dst before
    query number n"""
    wl = _base_workload(family)
    SA, SB = FAMILIES[family]
    base = A = State(family, wl, "base", _patterns(wl, 11), "pA", SA)
    B = A

    def update_rates(live, src, dst, n):
        live.update_edge_rates(dst.wl.edge_rates_csr)

    def set_model(live, src, dst, n):
        dst.set_model(live)

    def set_patterns(live, src, dst, n):
        dst.set_patterns(live)

    move = update_rates
    if change == "none":
        def move(live, src, dst, n):
            pass
    elif change == "rates":
        rates = wl.edge_rates_csr * np.random.default_rng(3).uniform(0.5, 2.0, wl.E)
        rates[_zero_rate_edge(wl, A.pats)] = 0.0
        B = A.but(wl=_variant(wl, edge_rates_csr=rates), wl_tag="ratesB")
    elif change == "mixture":
        ma, mb = _mixtures(family, wl)
        wa, wb = _variant(wl, mixture=ma), _variant(wl, mixture=mb)
        assert np.array_equal(wa.prepare()["Qn"], wb.prepare()["Qn"]) and np.array_equal(wa.prepare()["Qn_lo"], wb.prepare()["Qn_lo"])
        A, B, move = A.but(wl=wa, wl_tag="mixA"), A.but(wl=wb, wl_tag="mixB"), set_model
        assert B.C == A.C - 2 if wl.k == 4 else B.C == A.C - 1
    elif change == "root":
        rw = np.random.default_rng(5).uniform(0.05, 1.0, wl.k)
        A, B, move = (A.but(wl=_variant(wl, root="custom", root_custom=rw), wl_tag="rootA"),
                      A.but(wl=_variant(wl, root="none", root_custom=None), wl_tag="rootB"), set_model)
    elif change == "weights":
        B = A.but(weights=_weights(SA))

        def move(live, src, dst, n):
            live.set_site_weights(dst.weights)
    elif change == "patterns":
        rng = np.random.default_rng(7)
        extra = 17 - wl.nchar if wl.k == 4 else 1
        amb = rng.choice([0.0, 0.25, 0.5, 1.0], size=(extra, wl.k))
        amb[np.arange(extra), rng.integers(0, wl.k, extra)] = 0.75
        wb = _variant(wl, defs=np.vstack([wl.defs, amb]), nchar=wl.nchar + extra)
        assert wb.nchar == (17 if wl.k == 4 else wl.nchar + 1)
        A = A.but(weights=_weights(SA))
        B, move = A.but(wl=wb, wl_tag="defsB", pats=_patterns(wb, 12), pats_tag="pB", S=SB, weights=None), set_patterns
        assert np.max(B.pats) == wb.nchar - 1
    elif change == "layout":
        B, move = A.but(dense=True), set_patterns
    elif change == "options":
        A = A.but(S=OPTIONS_S.get(family, SA))
        B = A.but(options=(64, 1))

        def move(live, src, dst, n):
            dst.set_options(live)
    elif change == "tree":
        B = A.but(wl=_other_topology(wl), wl_tag="treeB")

        def move(live, src, dst, n):
            live.set_tree(dst.wl.indptr, dst.wl.indices, dst.wl.preorder)
            dst.set_model(live)
            dst.set_patterns(live)
    elif change == "fit":
        rates = _fit_rates(A)
        assert np.all(np.isfinite(rates)) and not np.array_equal(rates, wl.edge_rates_csr)
        B = A.but(wl=_variant(wl, edge_rates_csr=rates), wl_tag="fitB", update_from=wl.edge_rates_csr)

        def move(live, src, dst, n):
            if dst is B:
                got = live.fit_edge_rates(src.wl.edge_rates_csr, E_.FIT_EM, max_iter=2, ftol=0.0)[0]
                assert np.array_equal(got, rates), "the fit itself depends on what ran before it (query %d)" % n
            else:
                live.update_edge_rates(dst.wl.edge_rates_csr)
    elif change == "refused":
        def move(live, src, dst, n):
            with pytest.raises(E_.EngineError) as err:
                if n % 2 == 0:
                    bad = dst.wl.edge_rates_csr.copy()
                    bad[n % len(bad)] = np.inf
                    live.update_edge_rates(bad)
                else:
                    k0 = dst.wl.prepare()
                    Qn = k0["Qn"].copy()
                    Qn[n % wl.k, (n // 2) % wl.k] = np.nan
                    mode, rw = dst.wl.root_engine()
                    live.set_model(Qn, dst.wl.edge_rates_csr, k0["cat_rates"], k0["cat_prior"], mode, rw, Qn_lo=k0["Qn_lo"])
            assert err.value.code == E_.E_ARG
    else:
        assert change == "touch"
    return A, B, move, base


# ------------------------------------------------------------------------------------------------ the queries
def _second_order_pairs(eng):
    """plk_second_order with its {hi, lo} words as they come (Engine.second_order adds them)"""
    grad, hess = np.zeros((eng.E, 2)), np.zeros((eng.E, eng.E, 2))
    eng._check(eng._lib.plk_second_order(eng._h, ctypes.c_void_p(grad.ctypes.data), ctypes.c_void_p(hess.ctypes.data)))
    return grad, hess


def _run(eng, st, q):
    """-> (what the query returns, the PLK_INFO_* kernel values it leaves)"""
    info = lambda *items: tuple(eng.info(i) for i in items)
    if q == "ll":
        out = eng.ll()
        return out, info(E_.INFO_LL_KERNEL, E_.INFO_LL_VARIANT, E_.INFO_LL_FORM, E_.INFO_LL_FOLD, E_.INFO_PAIR_TABLES, E_.INFO_STACK_SLOTS)
    if q == "cat_posterior":
        return eng.cat_posterior(want_ll=True), info(E_.INFO_CAT_POSTERIOR_KERNEL, E_.INFO_CATEGORIES)
    if q in ("pair_sums", "rate_matrix_sens", "mixture_sens"):
        out = eng.edge_pair_sums() if q == "pair_sums" else eng.rate_matrix_sens() if q == "rate_matrix_sens" else eng.mixture_sens()
        kern = info(E_.INFO_MIXTURE_SENS_KERNEL if q == "mixture_sens" else E_.INFO_PAIR_SUMS_KERNEL)
        return out, kern + (info(E_.INFO_DOWN4_KERNEL) if kern[0] == FUSED4 else ())
    if q == "deriv":
        out = eng.deriv(edge_mask=st.emask)
    elif q == "marginal_sums":
        out = eng.marginal(per_site=False)[1:]
    elif q == "marginal":
        out = eng.marginal(node_mask=st.nmask)
    elif q == "expect":
        out = eng.edge_expect_multi(st.Ls, E_.COEF_PRIOR_RATE, Ls_lo=st.Ls_lo)
    else:
        assert q == "second_order"
        out = _second_order_pairs(eng)
    kern = info(E_.INFO_UPDOWN_KERNEL)
    return out, kern + (info(E_.INFO_UP4_PATH, E_.INFO_DOWN4_KERNEL) if kern[0] == FUSED4 else ())


def _same(a, b):
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.shape == b.shape and np.array_equal(a, b)
    if isinstance(a, tuple):
        return isinstance(b, tuple) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


def _finite(a):
    if isinstance(a, tuple):
        return all(_finite(x) for x in a)
    return a is None or bool(np.all(np.isfinite(a)))


def _fresh(st, q):
    """the query on a new engine that was brought to the state and runs nothing else"""
    e = E_.Engine(0)
    try:
        st.bring(e)
        return _run(e, st, q)
    finally:
        e.close()


def _check_family(family, st):
    """the family runs what its name says (one engine, the base state)"""
    e = E_.Engine(0)
    try:
        st.bring(e)
        ll = _run(e, st, "ll")[1]
        deriv = _run(e, st, "deriv")[1]
        pair = _run(e, st, "pair_sums")[1]
        post = _run(e, st, "cat_posterior")[1]
        second = _run(e, st, "second_order")[1]
    finally:
        e.close()
    got = (family, ll, deriv, pair, post, second)
    if family.startswith("k4"):
        assert ll[0] == FUSED4 and deriv[0] == FUSED4 and pair[0] == FUSED4 and post[0] == FUSED4 and second[0] == HESS4, got
        if family == "k4-stream":
            assert ll[2] == 1, got                                   # PLK_INFO_LL_FORM: streamed codes
        if family == "k4-deep":
            assert ll[5] == 5 and ll[1] == 1 and deriv[2] == 8, got   # stack need 5: assembly interpreter, k_down_fused4<8>
        if family == "k4-star":
            assert max(np.diff(st.wl.indptr)) > 32, got              # the wide node: k_range_check ahead of the stored-vector queries
    elif family == "k20":
        assert ll[0] == VEC and deriv[0] == VEC and pair[0] == GENERIC and post[0] == GENERIC and second[0] == GENERIC, got
    else:
        assert ll[0] == MFMA and deriv[0] == MFMA and pair[0] == GENERIC and post[0] == GENERIC and second[0] == GENERIC, got


# ------------------------------------------------------------------------------------------------ the oracle
_PREPARED, _ORACLE = {}, {}


def _oracle_values(oracle, st):
    """per-pattern ll, deriv, marginals and posteriors of a state's model and patterns (binary128), cached"""
    key = (st.family, st.wl_tag, st.pats_tag)
    if key in _ORACLE:
        return _ORACLE[key]
    wl = st.wl
    m = oracle.parse_model(wl.json_model(st.pats))
    pkey = (st.family, repr(wl.edges), wl.edge_rates_csr.tobytes(), repr(wl.mixture), repr(getattr(wl, "rate_mixture", None)))
    if pkey not in _PREPARED:
        _PREPARED[pkey] = oracle.prepare(m)                          # the binary128 exponentials: what k = 61 costs
    base = _PREPARED[pkey]
    rw = np.zeros(wl.k)
    if m.root_mode == 2:
        rw = np.array(m.root_custom, dtype=np.float64)
    elif m.root_mode == 4:
        rw = base["pi"].copy()
    w = dict(base, root_w=rw)                                        # as oracle.prepare sets it: the one entry the root prior moves
    codes_pn = np.ascontiguousarray(st.pats.T)
    B = wl.defs[codes_pn]
    ll, _ = oracle.site_ll(m, w, codes=codes_pn, defs=wl.defs, precise=2)
    assert np.all(np.isfinite(ll)), key
    post, rate, sll = catpost_cases.posteriors(oracle, m, w, precise=2, codes=codes_pn, defs=wl.defs)
    _ORACLE[key] = dict(C=int(w["C"]), ll=ll, deriv=oracle.site_deriv(m, w, B, precise=2), marg=oracle.site_marginal(m, w, B, precise=2),
                        post=post, rate=rate, sll=sll)
    return _ORACLE[key]


def _ld(x):
    return np.asarray(x[..., 0], dtype=LD) + np.asarray(x[..., 1], dtype=LD)


def _check_oracle(oracle, st, q, out, tag):
    ref = _oracle_values(oracle, st)
    sp = st.site_pat
    wts = np.ones(st.S) if st.weights is None else st.weights
    wl_, aw = wts.astype(LD), np.abs(wts)

    def wsum(v):                                                      # sum_s w_s v[pattern of s], in long double
        return np.tensordot(wl_, np.asarray(v, dtype=LD)[sp], axes=(0, 0))

    if q == "ll":
        site, (hi, lo) = out
        want = ref["ll"][sp]
        err = rel_err(site, want)
        print("%s: ll max rel err %.3g (bound %.3g)" % (tag, err, TOL))
        assert err <= TOL, tag
        bound = TOL * np.sum(np.abs(want)) if st.weights is None else SUM_TOL * float(np.sum(aw * np.maximum(1.0, np.abs(want))))
        assert abs((LD(hi) + LD(lo)) - wsum(ref["ll"])) <= bound, tag
    elif q == "deriv":
        got, sums = out
        sel = st.emask.astype(bool)
        want = ref["deriv"][sp]
        err = _row_err(got[:, sel], want[:, sel])
        print("%s: deriv max row err %.3g (bound %.3g)" % (tag, err, TOL))
        assert err <= TOL, tag
        assert np.all(got[:, ~sel] == 0.0) and np.all(sums[~sel] == 0.0), tag
        bound = SUM_TOL * np.sum(aw * np.max(np.abs(want), axis=1))
        assert np.max(np.abs(_ld(sums) - wsum(ref["deriv"]))[sel]) <= bound, tag
    elif q == "marginal_sums":
        sums, = out
        bound = SUM_TOL * np.tensordot(aw.astype(LD), np.abs(np.asarray(ref["marg"], dtype=LD))[sp], axes=(0, 0)) + PROB_ULP * np.sum(aw)
        assert np.all(np.abs(_ld(sums) - wsum(ref["marg"])) <= bound), tag
    else:
        assert q == "cat_posterior"
        gp, gr, psum, rsum, gll, lsum = out
        tol = catpost_cases.rtol(st.wl.E, st.wl.k, ref["C"])
        post, rate, sll = ref["post"][sp], ref["rate"][sp], ref["sll"][sp]
        catpost_cases.compare(tag, gp, gr, post, rate, tol)
        for c in range(ref["C"]):
            want = np.sum(wl_ * post[:, c])
            assert abs(_ld(psum[c]) - want) <= tol * want + 1e-300, tag
        want = np.sum(wl_ * rate)
        assert abs(_ld(np.asarray(rsum)) - want) <= tol * want, tag
        ll_bound = tol + 2.0 ** -52 * np.abs(sll)
        assert np.all(np.abs(gll.astype(LD) - sll) <= ll_bound), tag
        assert abs(_ld(np.asarray(lsum)) - np.sum(wl_ * sll)) <= np.sum(wl_ * ll_bound), tag


# ------------------------------------------------------------------------------------------------ the tests
_PREPARED_CASES = {}


def _case(oracle, family, change):
    """-> (states, move, fresh): the two states, the change, and the answers of the fresh engines, one engine per (state,
    query), grounded in the oracle; made once per (family, change) and shared by the two tests"""
    if (family, change) in _PREPARED_CASES:
        return _PREPARED_CASES[family, change]
    A, B, move, base = _states(family, change)
    states = (A, B)
    _check_family(family, base)
    fresh = {}
    for s in ((0,) if B is A else (0, 1)):
        for q in QUERIES:
            fresh[s, q] = _fresh(states[s], q)
            assert _finite(fresh[s, q][0]), (family, change, "AB"[s], q)
        for q in GROUNDED:
            _check_oracle(oracle, states[s], q, fresh[s, q][0], "%s %s state %s" % (family, change, "AB"[s]))
    if B is A:
        fresh.update({(1, q): fresh[0, q] for q in QUERIES})
    elif change in ("rates", "mixture", "root", "weights", "patterns", "tree", "fit"):
        # the change does move the answers: a walk between two equal states would say nothing about it
        assert not _same(fresh[0, "ll"][0], fresh[1, "ll"][0])
    _PREPARED_CASES[family, change] = (states, move, fresh)
    return _PREPARED_CASES[family, change]


def _live(tag, states, move, fresh, laps, steps):
    """one live engine, brought to A, runs the laps one after the other; laps(at) yields the (query, state) steps of the
    next lap for an engine in state `at`.  The change is applied wherever a step's state is not the engine's."""
    failures = []
    live = E_.Engine(0)
    try:
        states[0].bring(live)
        at, n, before = 0, 0, "set-up"
        for lap in laps:
            for qi, s in lap(at):
                q = QUERIES[qi]
                if s != at:
                    move(live, states[at], states[s], n)
                    at, before = s, before + ", change"
                got, want = _run(live, states[s], q), fresh[s, q]
                if got[1] != want[1]:
                    failures.append("query %d: %s at %s after %s: kernels %r, fresh engine %r" % (n, q, "AB"[s], before, got[1], want[1]))
                elif not _same(got[0], want[0]):
                    failures.append("query %d: %s at %s after %s: bits differ from a fresh engine" % (n, q, "AB"[s], before))
                before = "%s at %s" % (q, "AB"[at])
                n += 1
        assert n == steps
    finally:
        live.close()
    assert not failures, "%s: %d of %d answers differ:\n%s" % (tag, len(failures), n, "\n".join(failures[:40]))


@pytest.mark.parametrize("family,change", CASES, ids=["%s-%s" % c for c in CASES])
def test_query_order(oracle, family, change):
    """the change between every two queries: every (q1, q2) as "q1 at A, change, q2 at B" and the other way round"""
    states, move, fresh = _case(oracle, family, change)
    nq = len(QUERIES)
    # the second lap starts in B: the first one ends in A (an even number of changes), so a change stands between them too
    _live("%s %s" % (family, change), states, move, fresh, [lambda at: walk(nq, 0), lambda at: walk(nq, 1)], 2 * (nq * nq + 1))


# A change that leaves the state as it was has nothing to hold: "none" does nothing, and a refused call that dirtied
# something is seen by the query right after it in test_query_order.
HELD_CASES = [c for c in CASES if c[1] not in ("none", "refused")]


@pytest.mark.parametrize("family,change", HELD_CASES, ids=["%s-%s" % c for c in HELD_CASES])
def test_query_pairs_after_one_change(oracle, family, change):
    """the change before every second query only: every (q1, q2) as "change, q1, q2".  In test_query_order q2 always finds
    the engine freshly changed; here it finds what q1 left: plk_ll and plk_cat_posterior leave transition matrices
    without their derivatives, a derivative query a program without the ll formats.  A buffer that q2 wrongly takes as
    it is shows only if its last writer ran in the other state, so every visit that does not begin with one of FULL
    follows a visit that holds one."""
    states, move, fresh = _PREPARED_CASES.pop((family, change), None) or _case(oracle, family, change)
    _PREPARED_CASES.pop((family, change), None)
    nq = len(QUERIES)
    _live("%s %s" % (family, change), states, move, fresh, [lambda at: held_walk(nq, [QUERIES.index(q) for q in FULL], at)], 2 * nq * nq)
