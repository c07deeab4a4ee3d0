"""GPU: wide polytomies against the oracle.

A node vector is rescaled by the traversal program (OP_SCALE), never by a magnitude test inside a kernel, so what bounds
its range is the number of edge factors between two rescalings.  Before OP_SCALE could stand inside a node, a node with
m children took m factors at once: every shape below then leaves the double range in every rate category at most sites
(the ll kernels answered -inf, "site likelihood exactly 0", or a finite value with a large error).  Each case asserts on
the oracle's own numbers that it is such a case: at least half of its sites have ll < log(2^-1022), and every ll is above
log(1e-4900), so that the oracle (binary128, or the x87 format for k > 8 as in tests/test_gpu_kernel_families.py, both
with a 15-bit exponent) needs no rescaling of its own.

Shapes, leaf counts as used and the oracle's per-site ll range, measured on the CPU (the shapes were raised in steps of 10
leaves until the first condition held; never tuned against the engine):
  star90-short     root + 90 leaves, rates U[1e-6, 1e-5], k = 4, 4 gamma categories, 5 definitions, 129 sites
                   (70: no site qualifies, 80: 36 %, 90: 96 %); ll in [-832.1, -662.1]
  star90-short-C1  the same tree, one category; ll in [-904.3, -699.5] (98 %)
  star220-short    root + 220 leaves on short edges, 4 categories: the most the C++ k = 4 interpreter holds in LDS; ll in
                   [-2066.8, -1779.5] (all sites)
  star390          root + 390 leaves, rates U[0.05, 0.4], k = 4, 4 gamma categories, 129 sites
                   (300: none, 380: 26 %, 390: 57 %); ll in [-774.8, -650.9]
  star390-dense    the same with dense patterns
  wide-inside      caterpillar of 8 whose node at depth 3 also has 80 leaf children on short edges, 6 cherries and a unary
                   node, and data of its own (60: none, 70: 38 %, 80: 86 %); ll in [-914.8, -598.7]
  star200-k20      root + 200 leaves, 20 states, one category, 33 sites; ll in [-908.7, -836.8] (all sites)
  star150-k61      root + 150 leaves, 61 states, one category, 33 sites; ll in [-869.1, -828.8] (all sites)
(log(2^-1022) = -708.4; with four equally likely categories a site qualifies below -709.8, see _Case)

Log likelihoods and category posteriors interpret the program and are held to the oracle on every kernel of the shape's
row.  The queries that store node vectors (deriv, marginal, edge expectations, pair sums, rate-matrix and mixture
gradients, second order) keep one rescaling factor per node: on these shapes a device-side magnitude check finds a node
product below 2^-969 and they refuse (PLK_E_ARG, naming the query and the node) instead of miscomputing; the tests pin
that and that the engine answers the next ll query as before.  On benign nodes of the same kind -- a 40-leaf star, a
20-state one, a trifurcating root over three 8-leaf caterpillars (runs of 16 + 16 + 16), all on ordinary edges -- the same
queries are held to the oracle on every kernel family.  DESIGN.md section 6 lists the limit.

Tolerances: TOL and SUM_TOL of tests/test_gpu_kernel_families.py, the bound of tests/catpost_cases.py.
"""
import json

import numpy as np
import pytest

import catpost_cases
from helpers import oracle_model, rel_err, tree_workload
from test_gpu_kernel_families import SUM_TOL, TOL, _row_err, _wsum
from test_gpu_k4_stream import caterpillar

pytestmark = pytest.mark.gpu

LOG_TINY = -1022 * np.log(2.0)          # log of the smallest normal double
LOG_FLOOR = -4900 * np.log(10.0)
VEC, MFMA, GENERIC, FUSED4 = 4, 3, 2, 1
GAMMA4 = dict(gamma_shape=0.7, gamma_categories=4)


def star(m):
    """leaves 0 .. m-1 under the root m"""
    return [[m, i] for i in range(m)]


def _short(n, seed):
    return np.random.default_rng(seed).uniform(1e-6, 1e-5, n)


def _ordinary(n, seed):
    return np.random.default_rng(seed).uniform(0.05, 0.4, n)


WIDE_LEAVES, WIDE_NODE = 80, 11


def wide_inside():
    """caterpillar of 8 (leaves 0..7, internal 8..14, root 14): node 11, at depth 3, also gets WIDE_LEAVES leaf children on
    short edges, 6 cherries and a unary node over one leaf; node 11 carries data"""
    edges = caterpillar(8)
    rates = list(_ordinary(len(edges), 81))
    nxt = 15
    for _ in range(WIDE_LEAVES):
        edges.append([WIDE_NODE, nxt]); nxt += 1
    rates += list(_short(WIDE_LEAVES, 82))
    for _ in range(6):
        edges += [[WIDE_NODE, nxt], [nxt, nxt + 1], [nxt, nxt + 2]]; nxt += 3
    edges += [[WIDE_NODE, nxt], [nxt, nxt + 1]]
    rates += list(_ordinary(len(edges) - len(rates), 83))
    return edges, rates


def _make(name):
    """-> (workload, number of sites)"""
    if name in ("star90-short", "star90-short-C1"):
        m = 90
        return tree_workload(4, star(m), _short(m, 70), root="equilibrium", seed=9070, nchar=5,
                             gamma=GAMMA4 if name == "star90-short" else None, name=name), 129
    if name == "star220-short":
        return tree_workload(4, star(220), _short(220, 71), root="equilibrium", seed=9220, nchar=5, gamma=GAMMA4, name=name), 129
    if name in ("star390", "star390-dense"):
        return tree_workload(4, star(390), _ordinary(390, 300), root="equilibrium", seed=9300, gamma=GAMMA4, nchar=5, name=name), 129
    if name == "wide-inside":
        edges, rates = wide_inside()
        return tree_workload(4, edges, rates, root="equilibrium", seed=9011, gamma=GAMMA4, nchar=5, data_nodes=(WIDE_NODE,), name=name), 129
    if name == "star200-k20":
        return tree_workload(20, star(200), _ordinary(200, 200), root="equilibrium", seed=9200, name=name), 33
    if name == "star150-k61":
        return tree_workload(61, star(150), _ordinary(150, 150), root="equilibrium", seed=9150, name=name), 33
    raise ValueError(name)


def _codes(wl, S, seed):
    """an observed state on every leaf and data node (no missing data: every leaf is a factor), the all-ones row elsewhere"""
    rng = np.random.default_rng([seed, S])
    codes = np.full((wl.N, S), wl.k, dtype=np.uint8)
    leaf = wl.indptr[1:] == wl.indptr[:-1]
    for a in range(wl.N):
        if leaf[a] or a in wl.data_nodes:
            codes[a] = rng.integers(0, wl.k, S)
    return codes


class _Case:
    """one shape: workload, codes, weights with zeros, and the oracle's per-site ll (built once per module)"""

    def __init__(self, oracle, name):
        self.name = name
        self.wl, self.S = _make(name)
        self.codes = _codes(self.wl, self.S, seed=len(name))
        self.precise = 2 if self.wl.k <= 8 else 1
        self.m, self.w = oracle_model(oracle, self.wl, self.codes)
        self.ll, _ = oracle.site_ll(self.m, self.w, codes=np.ascontiguousarray(self.codes.T), defs=self.wl.defs, precise=self.precise)
        self.weights = np.random.default_rng(self.S).uniform(0.25, 4.0, self.S)
        self.weights[::7] = 0.0
        self._post = None
        # the case is a case, on the oracle's own numbers: L = sum_c prior_c L_c, so L_c <= L / prior_c, and a site whose ll is
        # below log(2^-1022) + log(min prior) has every category's likelihood below the smallest normal double
        prior = np.asarray(self.w["cat_prior"], dtype=float)
        self.log_tiny_all = LOG_TINY + float(np.log(np.min(prior[prior > 0])))
        assert np.mean(self.ll < self.log_tiny_all) >= 0.5, name
        assert self.ll.min() > LOG_FLOOR, name

    def posteriors(self, oracle):
        if self._post is None:
            post, rate, sll = catpost_cases.posteriors(oracle, self.m, self.w, precise=self.precise,
                                                       codes=np.ascontiguousarray(self.codes.T), defs=self.wl.defs)
            self._post = (self.m, self.w, post, rate, sll)
        return self._post

    def upload(self, eng, dense=False):
        self.wl.setup_engine(eng)
        if dense:
            eng.set_patterns_dense(np.ascontiguousarray(self.wl.defs[self.codes.T].transpose(1, 2, 0)))
        else:
            eng.set_patterns_codes(self.codes, self.wl.defs)
        eng.set_site_weights(None)


_CASES = {}


@pytest.fixture
def case(oracle, request):
    name = request.node.callspec.params["shape"]
    base = "star390" if name == "star390-dense" else name
    if base not in _CASES:
        _CASES[base] = _Case(oracle, base)
    return _CASES[base]


def _defaults():
    from phyly_amd import engine as E
    return {E.OPT_FORCE_GENERIC: 0, E.OPT_SITE_CHUNK: 0, E.OPT_MFMA: 1, E.OPT_UP_NODES: 2, E.OPT_PAIR_TABLES: 1, E.OPT_VEC_REG_STACK: 1,
            E.OPT_MFMA_NS2: 0, E.OPT_FUSED_ASM: 1, E.OPT_FUSED_NS: 0}


def _set_options(eng, opts):
    for o, v in _defaults().items():
        eng.set_option(o, opts.get(o, v))


@pytest.fixture(scope="module")
def eng():
    from phyly_amd.engine import Engine
    e = Engine(0)
    yield e
    _set_options(e, {})
    e.close()


def _kernels(shape):
    """-> [(tag, options, expected (kernel, variant, form); None = not checked)] in the order of the shape's row"""
    from phyly_amd import engine as E
    if shape in ("star90-short", "star90-short-C1"):
        return [("stream", {E.OPT_PAIR_TABLES: 7}, (FUSED4, 6, 1)), ("tile", {E.OPT_PAIR_TABLES: 6}, (FUSED4, 6, 0)),
                ("asm", {E.OPT_PAIR_TABLES: 0}, (FUSED4, 1, None)), ("cpp-ns2", {E.OPT_FUSED_NS: 2}, (FUSED4, 3, None))]
    if shape == "star220-short":
        # the most leaves whose staged rows the C++ interpreter holds with two sites per lane (512 bytes a row): six rescalings
        # inside the root
        return [("cpp-ns2", {E.OPT_FUSED_NS: 2}, (FUSED4, 3, None)), ("cpp", {E.OPT_FUSED_ASM: 0, E.OPT_PAIR_TABLES: 0}, (FUSED4, 3, None)),
                ("asm", {E.OPT_PAIR_TABLES: 0}, (FUSED4, 1, None))]
    if shape == "star390":
        # (the C++ interpreter's staged rows of 390 leaves, 256 or 512 bytes each, do not fit the LDS: it runs on star90-short)
        return [("asm", {}, (FUSED4, 1, None)), ("generic", {E.OPT_FORCE_GENERIC: 1}, (GENERIC, None, None))]
    if shape == "wide-inside":
        return [("plan", {}, None)]
    if shape == "star200-k20":
        return [("vec", {}, (VEC, None, None))]
    if shape == "star150-k61":
        return [("mfma", {}, (MFMA, None, None))]
    if shape == "star390-dense":
        return [("dense", {}, (GENERIC, None, None))]
    raise ValueError(shape)


LL_SHAPES = ["star90-short", "star90-short-C1", "star220-short", "star390", "wide-inside", "star200-k20", "star150-k61", "star390-dense"]


@pytest.mark.parametrize("shape", LL_SHAPES)
def test_ll(eng, case, shape):
    """per-site ll and the weighted sum against the oracle on every kernel of the shape's row; the kernels of one row toggled
    in one engine: stream and tile forms bit for bit, the others within TOL of each other"""
    from phyly_amd import engine as E
    want = case.ll
    case.upload(eng, dense=shape == "star390-dense")
    seen = {}
    try:
        for rnd in range(2):                     # there and back: each kernel after each other one
            for tag, opts, expect in _kernels(shape):
                _set_options(eng, opts)
                eng.set_site_weights(None)
                got, (hi, lo) = eng.ll()
                got = got.copy()
                ran = (eng.info(E.INFO_LL_KERNEL), eng.info(E.INFO_LL_VARIANT), eng.info(E.INFO_LL_FORM))
                if expect is None:
                    assert ran[0] != GENERIC, (shape, ran)
                else:
                    assert all(e is None or e == r for e, r in zip(expect, ran)), (shape, tag, ran)
                assert np.all(np.isfinite(got)), (shape, tag)
                assert rel_err(got, want) <= TOL, (shape, tag)
                assert abs((hi + lo) - float(np.sum(want.astype(np.longdouble)))) <= TOL * np.sum(np.abs(want)), (shape, tag)
                eng.set_site_weights(case.weights)
                gw, (hi, lo) = eng.ll()
                assert np.array_equal(gw, got), (shape, tag)
                bound = SUM_TOL * float(np.sum(np.abs(case.weights) * np.maximum(1.0, np.abs(want))))
                assert abs((hi + lo) - float(_wsum(want, case.weights))) <= bound, (shape, tag)
                if tag in seen:
                    assert np.array_equal(seen[tag], got), (shape, tag, "not reproducible after a toggle")
                seen[tag] = got
        if "stream" in seen:
            assert np.array_equal(seen["stream"], seen["tile"]), shape
        tags = list(seen)
        for a in tags[1:]:
            assert rel_err(seen[a], seen[tags[0]]) <= TOL, (shape, a)
    finally:
        eng.set_site_weights(None)
        _set_options(eng, {})


def _families(k):
    """-> [(tag, options, PLK_INFO_UPDOWN_KERNEL)]: the kernel families a stored-vector query with k states can be sent to"""
    from phyly_amd import engine as E
    if k == 4:
        return [("k4", {}, FUSED4), ("generic", {E.OPT_FORCE_GENERIC: 1}, GENERIC)]
    if k <= 20:
        return [("vec", {}, VEC), ("mfma", {E.OPT_MFMA: 2}, MFMA), ("mfma-up-nodes", {E.OPT_MFMA: 2, E.OPT_UP_NODES: 3}, MFMA),
                ("generic", {E.OPT_FORCE_GENERIC: 1}, GENERIC)]
    return [("mfma", {}, MFMA), ("mfma-up-nodes", {E.OPT_UP_NODES: 3}, MFMA), ("generic", {E.OPT_FORCE_GENERIC: 1}, GENERIC)]


def _wide_node(wl):
    deg = np.diff(wl.indptr)
    return int(np.argmax(deg)), int(np.max(deg))


def _refused(eng, case, call, query):
    """the query refuses with PLK_E_ARG, names itself, the magnitude and the wide node; the engine then answers ll as the
    oracle does"""
    from phyly_amd import engine as E
    node, deg = _wide_node(case.wl)
    with pytest.raises(E.EngineError) as ei:
        call()
    msg = str(ei.value)
    assert ei.value.code == E.E_ARG, msg
    assert query in msg and "2^-969" in msg and ("node %d with %d children" % (node, deg)) in msg, msg
    got, _ = eng.ll()
    assert rel_err(got, case.ll) <= TOL, (case.name, query)


UPDOWN_SHAPES = ["star90-short", "wide-inside", "star390", "star200-k20", "star150-k61"]
QUERY_SHAPES = ["star90-short", "wide-inside", "star200-k20"]


def _third_of_wide_node(wl):
    """edge mask (CSR order) that keeps every third edge of the widest node"""
    node, _ = _wide_node(wl)
    mask = np.zeros(wl.E, dtype=np.int32)
    mask[np.arange(wl.indptr[node], wl.indptr[node + 1])[::3]] = 1
    return mask


@pytest.mark.parametrize("shape", UPDOWN_SHAPES)
def test_underflowing_products_are_refused(eng, case, shape):
    """deriv, marginal and edge expectations (per-site, site-summed, masked) on the shapes whose node products leave the
    double range: the device-side magnitude check refuses them, whatever family the query would have taken"""
    from phyly_amd import engine as E
    case.upload(eng)
    k = case.wl.k
    L = np.random.default_rng(k).uniform(-1, 1, (k, k))
    mask = _third_of_wide_node(case.wl)
    nmask = (np.arange(case.wl.N) % 3 == 0).astype(np.int32)
    try:
        for tag, opts, _ in _families(k):
            _set_options(eng, opts)
            _refused(eng, case, lambda: eng.deriv(), "plk_deriv")
            _refused(eng, case, lambda: eng.deriv(edge_mask=mask, per_site=False), "plk_deriv")
            _refused(eng, case, lambda: eng.marginal(), "plk_marginal")
            _refused(eng, case, lambda: eng.marginal(node_mask=nmask, per_site=False), "plk_marginal")
            _refused(eng, case, lambda: eng.edge_expect(L, E.COEF_PRIOR, edge_mask=mask), "plk_edge_expect")
    finally:
        _set_options(eng, {})


@pytest.mark.parametrize("shape", QUERY_SHAPES)
def test_underflowing_products_are_refused_by_the_sum_queries(eng, case, shape):
    from phyly_amd import engine as E
    case.upload(eng)
    eng.set_site_weights(case.weights)
    try:
        for opts in ({}, {E.OPT_FORCE_GENERIC: 1}):
            _set_options(eng, opts)
            _refused(eng, case, lambda: eng.edge_pair_sums(), "plk_edge_pair_sums")
            _refused(eng, case, lambda: eng.rate_matrix_sens(), "plk_rate_matrix_sens")
            _refused(eng, case, lambda: eng.mixture_sens(), "plk_mixture_sens")
    finally:
        eng.set_site_weights(None)
        _set_options(eng, {})


@pytest.mark.parametrize("shape", ["star90-short"])
def test_second_order(eng, case, shape):
    """the k = 4 pass and the generic passes (33 sites): refused before the first of the E + 1 passes"""
    from phyly_amd import engine as E
    case.wl.setup_engine(eng)
    eng.set_patterns_codes(np.ascontiguousarray(case.codes[:, :33]), case.wl.defs)
    want33 = case.ll[:33]
    node, deg = _wide_node(case.wl)
    try:
        for opts in ({}, {E.OPT_FORCE_GENERIC: 1}):
            _set_options(eng, opts)
            for call in (eng.second_order, eng.hess):
                with pytest.raises(E.EngineError) as ei:
                    call()
                assert ei.value.code == E.E_ARG and "plk_second_order" in str(ei.value), str(ei.value)
                assert ("node %d with %d children" % (node, deg)) in str(ei.value)
                got, _ = eng.ll()
                assert rel_err(got, want33) <= TOL
    finally:
        _set_options(eng, {})


# ---------------------------------------------------------------------------------------------------------------------
# benign nodes that the program rescales inside (more than 32 edge factors in one run, tests/progcheck_main.cpp builds the
# same two shapes and asserts it): ordinary branch lengths, products far inside the double range -- every stored-vector
# query answers, on every family, to the bars of tests/test_gpu_kernel_families.py
# ---------------------------------------------------------------------------------------------------------------------

def three_caterpillars():
    """a root (45) over three 8-leaf caterpillars (15 nodes each, tops 14, 29, 44): every other node has two children, the
    root's three runs of 16 edge factors make 48"""
    edges = []
    for c in range(3):
        edges += [[p + 15 * c, q + 15 * c] for p, q in caterpillar(8)]
    return edges + [[45, 14], [45, 29], [45, 44]]


def _make_benign(name):
    if name == "star40":
        return tree_workload(4, star(40), _ordinary(40, 40), root="equilibrium", seed=9040, gamma=GAMMA4, nchar=5, name=name), 129
    if name == "trifurcating-root":
        edges = three_caterpillars()
        return tree_workload(4, edges, _ordinary(len(edges), 48), root="equilibrium", seed=9048, gamma=GAMMA4, nchar=5, name=name), 129
    if name == "star40-k20":
        return tree_workload(20, star(40), _ordinary(40, 41), root="equilibrium", seed=9041, name=name), 65
    raise ValueError(name)


class _Benign:
    def __init__(self, oracle, name):
        self.name = name
        self.wl, self.S = wl, S = _make_benign(name)
        self.codes = _codes(wl, S, seed=len(name))
        self.precise = 2 if wl.k <= 8 else 1
        self.m, self.w = oracle_model(oracle, wl, self.codes)
        B = wl.defs[self.codes.T]
        self.ll, _ = oracle.site_ll(self.m, self.w, codes=np.ascontiguousarray(self.codes.T), defs=wl.defs, precise=self.precise)
        assert self.ll.min() > -400                     # benign: nowhere near the edge of the double range (-708)
        self.deriv = oracle.site_deriv(self.m, self.w, B, precise=self.precise)
        self.marg = oracle.site_marginal(self.m, self.w, B, precise=self.precise)
        rng = np.random.default_rng(wl.k + S)
        self.L = rng.uniform(-1, 1, (wl.k, wl.k))
        self.xmask = np.zeros(wl.E, dtype=np.int32)
        self.xmask[rng.choice(wl.E, size=3, replace=False)] = 1
        F = oracle.frechet(self.m, self.w, self.L, 1.0, False, self.xmask, precise=self.precise)
        self.expect = {c: oracle.site_edge_expect(self.m, self.w, B, F, c, self.xmask, precise=self.precise) for c in (0, 1)}
        self.weights = rng.choice([-1.0, 1.0], S) * 10.0 ** rng.uniform(-3, 3, S)


_BENIGN = {}
BENIGN = ["star40", "trifurcating-root", "star40-k20"]


def _benign_cases():
    ks = {"star40": 4, "trifurcating-root": 4, "star40-k20": 20}
    return [pytest.param(n, f[0], id="%s-%s" % (n, f[0])) for n in BENIGN for f in _families(ks[n])]


@pytest.fixture
def benign(oracle, request):
    name = request.node.callspec.params["shape"]
    if name not in _BENIGN:
        _BENIGN[name] = _Benign(oracle, name)
    return _BENIGN[name]


@pytest.mark.parametrize("shape,family", _benign_cases())
def test_benign_wide_nodes_are_answered(eng, benign, shape, family):
    """ll, deriv, marginal and edge expectations against the oracle: per site, weighted sums, masks"""
    from phyly_amd import engine as E
    from test_gpu_kernel_families import PROB_ULP
    wl, wts = benign.wl, benign.weights
    _, opts, udk = next(f for f in _families(wl.k) if f[0] == family)
    wl.setup_engine(eng)
    eng.set_patterns_codes(benign.codes, wl.defs)
    emask = _third_of_wide_node(wl)
    esel = emask.astype(bool)
    nmask = (np.arange(wl.N) % 3 == 0).astype(np.int32)
    nsel = nmask.astype(bool)
    try:
        _set_options(eng, opts)
        eng.set_site_weights(wts)
        got, _ = eng.ll()
        assert rel_err(got, benign.ll) <= TOL
        # derivatives
        want = benign.deriv
        got, sums = eng.deriv()
        assert eng.info(E.INFO_UPDOWN_KERNEL) == udk
        assert _row_err(got, want) <= TOL
        bound = SUM_TOL * np.sum(np.abs(wts) * np.max(np.abs(want), axis=1))
        assert np.max(np.abs((sums[:, 0] + sums[:, 1]) - _wsum(want, wts).astype(float))) <= bound
        got, sums = eng.deriv(edge_mask=emask)
        assert _row_err(got[:, esel], want[:, esel]) <= TOL
        assert np.all(got[:, ~esel] == 0.0) and np.all(sums[~esel] == 0.0)
        # marginals
        want = benign.marg
        got, sums = eng.marginal()
        assert eng.info(E.INFO_UPDOWN_KERNEL) == udk
        assert np.max(np.abs(got - want)) <= TOL
        ref_sum = _wsum(want, wts).astype(float)
        bound = SUM_TOL * _wsum(np.abs(want), np.abs(wts)).astype(float) + PROB_ULP * np.sum(np.abs(wts))
        assert np.all(np.abs((sums[..., 0] + sums[..., 1]) - ref_sum) <= bound)
        _, fused = eng.marginal(per_site=False)
        assert np.all(np.abs((fused[..., 0] + fused[..., 1]) - ref_sum) <= bound)
        got, sums = eng.marginal(node_mask=nmask)
        assert np.max(np.abs(got[:, nsel] - want[:, nsel])) <= TOL
        assert np.all(got[:, ~nsel] == 0.0) and np.all(sums[~nsel] == 0.0)
        # edge expectations
        eng.set_site_weights(None)
        xsel = benign.xmask.astype(bool)
        for coef, mode in ((0, E.COEF_PRIOR), (1, E.COEF_PRIOR_RATE_EDGE)):
            want = benign.expect[coef]
            got, sums = eng.edge_expect(benign.L, mode, edge_mask=benign.xmask)
            assert _row_err(got[:, xsel], want[:, xsel]) <= TOL, mode
            tot = (sums[:, 0] + sums[:, 1])[xsel]
            bound = SUM_TOL * np.sum(np.max(np.abs(want[:, xsel]), axis=1))
            assert np.max(np.abs(tot - want[:, xsel].astype(np.longdouble).sum(axis=0).astype(float))) <= bound, mode
    finally:
        eng.set_site_weights(None)
        _set_options(eng, {})


@pytest.mark.parametrize("shape", BENIGN)
def test_benign_wide_nodes_sum_queries(eng, benign, shape):
    """second order, mixture gradient and pair sums are answered and agree with what the oracle-checked queries give: the
    gradient of plk_second_order is the edge sums of plk_deriv, sum_c r_c rate_out[c] = sum_e t_e deriv_e (include/plk.h),
    and the pair sums of an edge add up, over states and categories, to the sum of the weights"""
    from phyly_amd import engine as E
    wl = benign.wl
    wts = np.abs(benign.weights)
    wl.setup_engine(eng)
    eng.set_patterns_codes(np.ascontiguousarray(benign.codes[:, :33]), wl.defs)
    eng.set_site_weights(wts[:33])
    want = _wsum(benign.deriv[:33], wts[:33]).astype(float)
    scale = float(np.sum(wts[:33, None] * np.abs(benign.deriv[:33]), axis=0).max())
    try:
        for opts in ({}, {E.OPT_FORCE_GENERIC: 1}):
            _set_options(eng, opts)
            grad, hess = eng.second_order()
            assert np.max(np.abs(grad - want)) <= 1e-11 * scale, shape
            assert np.all(np.isfinite(hess))
            prior_out, rate_out = eng.mixture_sens()
            cr = wl.prepare()["cat_rates"]
            lhs = float(np.sum(cr * (rate_out[:, 0] + rate_out[:, 1])))
            rhs = float(np.sum(wl.edge_rates_csr * want))
            assert abs(lhs - rhs) <= 1e-11 * float(np.sum(wl.edge_rates_csr) * scale), shape
            W, root = eng.edge_pair_sums()
            assert np.all(np.isfinite(W)) and np.all(np.isfinite(root))
    finally:
        eng.set_site_weights(None)
        _set_options(eng, {})


QUERY_SHAPES = ["star90-short", "wide-inside", "star200-k20"]


@pytest.mark.parametrize("shape", QUERY_SHAPES)
def test_cat_posterior(eng, oracle, case, shape):
    """posteriors, posterior mean rates and the ll by-product against the oracle: the k = 4 kernel and the generic one (the
    bound of tests/catpost_cases.py, the bars of tests/test_gpu_cat_posterior.py)"""
    from phyly_amd import engine as E
    ref = case.posteriors(oracle)
    case.upload(eng)
    try:
        kernels = [(1, {}), (2, {E.OPT_FORCE_GENERIC: 1})] if case.wl.k == 4 else [(2, {})]
        for kernel, opts in kernels:
            _set_options(eng, opts)
            # the oracle in the x87 format (k > 8): its 64-bit mantissa costs the same operation count once more at 2^-64
            extra = catpost_cases.rtol(case.wl.E, case.wl.k, int(case.w["C"])) * 2.0 ** -11 if case.precise == 1 else 0.0
            gp, gr, _, _ = catpost_cases.check_engine(eng, oracle, case.wl, case.codes, "%s kernel %d" % (shape, kernel), kernel,
                                                      precise=case.precise, extra_tol=extra, ref=ref, site_weights=case.weights)
            assert np.all(np.isfinite(gp)) and np.all(np.isfinite(gr))
    finally:
        eng.set_site_weights(None)
        _set_options(eng, {})


@pytest.mark.parametrize("shape", ["star90-short"])
def test_json_commands(oracle, case, shape, capfd):
    """arbplf_ll on the star answers as the oracle does (not "site likelihood exactly 0"); arbplf_deriv and arbplf_marginal
    fail with the refusal on stderr, and the next ll query is answered"""
    import arbplf
    from test_gpu_differential import _check
    md = case.wl.json_model(case.codes[:, :40])
    q = json.dumps({"model_and_data": md})
    want = json.loads(oracle.arbplf_ll(q))
    assert all(np.isfinite(r[-1]) for r in want["data"])
    assert sum(r[-1] < LOG_TINY for r in want["data"]) >= len(want["data"]) // 2
    _check("ll", json.loads(arbplf.arbplf_ll(q)), want)
    agg = json.dumps({"model_and_data": md, "site_reduction": {"aggregation": "sum"}})
    _check("ll", json.loads(arbplf.arbplf_ll(agg)), json.loads(oracle.arbplf_ll(agg)))
    capfd.readouterr()
    for fn in (arbplf.arbplf_deriv, arbplf.arbplf_marginal):
        with pytest.raises(RuntimeError):
            fn(q)
        err = capfd.readouterr().err
        assert "with 90 children" in err and "2^-969" in err, err
        _check("ll", json.loads(arbplf.arbplf_ll(q)), want)


def test_definitions_scaled_by_2_to_minus_30(eng, oracle):
    """the envelope of DESIGN.md section 6: at most PLK_SCALE_RUN = 32 factors between two rescalings, each at least 2^-31.
    On the 40-taxon caterpillar (at most 16 factors per run) every definition row is scaled by 2^-30, the all-ones row
    included, so every one of the N nodes multiplies 2^-30 in: per-site ll moves by exactly N * 30 ln 2, derivatives and
    marginals do not move.  The unscaled run is held to the oracle."""
    from test_gpu_k4_stream import _codes as cat_codes, _workload
    from phyly_amd import engine as E
    wl = _workload(caterpillar(40), seed=40)
    S = 129
    codes = cat_codes(wl, S, seed=30, missing=0.1)
    wl.setup_engine(eng)
    _set_options(eng, {})
    eng.set_patterns_codes(codes, wl.defs)
    eng.set_site_weights(None)
    ll0, _ = eng.ll()
    ll0 = ll0.copy()
    d0, m0 = eng.deriv()[0].copy(), eng.marginal()[0].copy()
    m, w = oracle_model(oracle, wl, codes)
    want, _ = oracle.site_ll(m, w, codes=np.ascontiguousarray(codes.T), defs=wl.defs, precise=2)
    assert rel_err(ll0, want) <= TOL
    eng.set_patterns_codes(codes, wl.defs * 2.0 ** -30)
    ll1, _ = eng.ll()
    assert eng.info(E.INFO_LL_KERNEL) == FUSED4
    shift = wl.N * 30 * np.log(2.0)
    assert rel_err(ll1, ll0 - shift) <= TOL
    d1, m1 = eng.deriv()[0], eng.marginal()[0]
    assert _row_err(d1, d0) <= TOL
    assert np.max(np.abs(m1 - m0)) <= TOL
    eng.set_option(E.OPT_FORCE_GENERIC, 1)
    try:
        ll2, _ = eng.ll()
        assert eng.info(E.INFO_LL_KERNEL) == GENERIC
        assert rel_err(ll2, ll0 - shift) <= TOL
        assert _row_err(eng.deriv()[0], d0) <= TOL
        assert np.max(np.abs(eng.marginal()[0] - m0)) <= TOL
    finally:
        eng.set_option(E.OPT_FORCE_GENERIC, 0)
