"""GPU: plk_place_ll / arbplf-place against the oracle's ll of the tree with the query attached (tests/place_cases.py
rewrites the model document).  Bars: per site |d| <= 1e-12 max(1, |ll'|); sums within 1e-12 of the long double host sum
of the reference values: the bars of tests/test_gpu_nni.py."""
import json
import os
import subprocess

import numpy as np
import pytest

import mixsens_cases
import place_cases as cases
from helpers import GOLDEN, K4_MODELS, QUERY_MODEL, family_workload, load_json, query_workload
from phyly_amd import engine as E_, synth
from phyly_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FELSENSTEIN = os.path.join(GOLDEN, "examples", "Felsenstein.2004.fig.16.4", "ll", "in.json")
SPLIT, PENDANT = 0.3, 0.07
_refs = {}


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _case(oracle, key, build):
    """(md, Reference, character_data [S][N]) built once per module"""
    if key not in _refs:
        md = build()
        _refs[key] = (md, cases.Reference(oracle, md), np.asarray(md["character_data"]))
    return _refs[key]


def _dd(sums):
    sums = np.asarray(sums)
    return np.asarray(sums[..., 0], dtype=cases.LD) + np.asarray(sums[..., 1], dtype=cases.LD)


def _check_rows(ref, Q, edges, got, sums, wt, split=SPLIT, pendant=PENDANT):
    """got [Q][n][S], sums [Q][n][2] against the oracle; Q [nq][S] character indices, edges in user indices"""
    worst = 0.0
    for qi, q in enumerate(Q):
        for i, e in enumerate(edges):
            want = ref.place(e, q, split, pendant)
            err = cases.site_err(got[qi, i], want)
            worst = max(worst, err)
            assert err <= cases.SITE_TOL, (qi, e, err)
            if sums is not None and np.all(np.isfinite(want)):       # a row with an impossible site has no finite sum to meet
                ws = cases.weighted_sum(want, wt)
                assert abs(_dd(sums)[qi, i] - ws) <= cases.SUM_TOL * abs(ws), (qi, e, float(_dd(sums)[qi, i]), float(ws))
    return worst


def _dense_queries(md, Q):
    """[Q][k][S] observation rows of queries given as character indices"""
    return np.ascontiguousarray(np.transpose(np.asarray(md["character_definitions"], dtype=float)[np.asarray(Q, dtype=int)], (0, 2, 1)))


# ---------------------------------------------------------------- the k = 4 models
@pytest.mark.parametrize("S", [1, 65, 257])
@pytest.mark.parametrize("name", list(K4_MODELS) + [QUERY_MODEL])
def test_k4_models(eng, oracle, name, S):
    md, ref, data = _case(oracle, (name, S), lambda: cases.workload_doc(query_workload(name), S, seed=S))
    Q = cases.queries(md, data, seed=S)
    assert Q.shape == (3, S)
    user = list(range(len(md["edges"]))) if S == 65 else cases.sample_edges(md, 16, seed=S)
    kinds = cases.edge_kinds(md)
    assert set().union(*kinds.values()) <= set().union(*(kinds[e] for e in user))      # every kind of edge the tree has
    if name in ("irregular", "wide"):
        assert set().union(*(kinds[e] for e in user)) == {"root", "leaf", "data", "multi", "zero"}
    csr = cases.csr_edges(md, user)
    C = ref.w["C"]
    wt = cases.six_decade_weights(S, 3 + S)
    for layout in ("compact", "generic", "dense"):
        mixsens_cases.setup_engine(eng, oracle, md)
        if layout == "dense":
            eng.set_patterns_dense(np.ascontiguousarray(np.transpose(ref.m.B, (1, 2, 0))))
        eng.set_option(E_.OPT_FORCE_GENERIC, 1 if layout == "generic" else 0)
        kw = dict(q_dense=_dense_queries(md, Q)) if layout == "dense" else dict(q_codes=Q)
        try:
            got, sums = eng.place_ll(edges=csr, split=SPLIT, pendant_rate=PENDANT, **kw)
            k4 = layout == "compact" and C <= 4
            assert eng.info(E_.INFO_PLACE_KERNEL) == (1 if k4 else 2), (name, layout)
            worst = _check_rows(ref, Q, user, got, sums, None)
            eng.set_site_weights(wt)
            got_w, sums_w = eng.place_ll(edges=csr, split=SPLIT, pendant_rate=PENDANT, **kw)
            assert np.array_equal(got, got_w)                   # weights touch the sums only
            _check_rows(ref, Q, user, got_w, sums_w, wt)
            print("%s S=%d %s: %d edges, worst site error %.2e" % (name, S, layout, len(user), worst))
        finally:
            eng.set_site_weights(None)
            eng.set_option(E_.OPT_FORCE_GENERIC, 0)


# ---------------------------------------------------------------- other state counts
@pytest.mark.parametrize("k", [2, 5, 13, 27, 48])
def test_family_models(eng, oracle, k):
    md, ref, data = _case(oracle, ("family", k), lambda: cases.workload_doc(family_workload(k), 65, seed=k))
    Q = cases.queries(md, data, seed=k)[[0, 2]]
    user = cases.sample_edges(md, 12, seed=k)
    mixsens_cases.setup_engine(eng, oracle, md)
    wt = cases.six_decade_weights(65, k)
    eng.set_site_weights(wt)
    try:
        got, sums = eng.place_ll(q_codes=Q, edges=cases.csr_edges(md, user), split=SPLIT, pendant_rate=PENDANT)
    finally:
        eng.set_site_weights(None)
    assert eng.info(E_.INFO_PLACE_KERNEL) == 2
    print("k=%d: %d edges, worst site error %.2e" % (k, len(user), _check_rows(ref, Q, user, got, sums, wt)))


# ---------------------------------------------------------------- carried-over scale factors
@pytest.mark.parametrize("k", [4, 13])
def test_ladder_of_200_leaves(eng, oracle, k):
    """edge rates near 1 and observation rows scaled by 1e-4: every site likelihood is far below 2^-1022"""
    md, ref, data = _case(oracle, ("ladder", k), lambda: cases.ladder_doc(200, 33, seed=40 + k, k=k, C=2, leaf_scale=1e-4))
    assert np.max(ref.current()) < -1022 * np.log(2.0) - 100
    Q = cases.queries(md, data, seed=k)[:2]
    user = cases.sample_edges(md, 16, seed=k, spread=True)
    mixsens_cases.setup_engine(eng, oracle, md)
    got, sums = eng.place_ll(q_codes=Q, edges=cases.csr_edges(md, user), split=SPLIT, pendant_rate=PENDANT)
    assert eng.info(E_.INFO_PLACE_KERNEL) == (1 if k == 4 else 2)
    assert np.all(np.isfinite(got))
    print("ladder k=%d: worst site error %.2e" % (k, _check_rows(ref, Q, user, got, sums, None)))


# ---------------------------------------------------------------- extremes of the parameters
@pytest.mark.parametrize("pendant", [0.0, 50.0])
@pytest.mark.parametrize("split", [0.0, 1.0, 0.5])
def test_extreme_parameters(eng, oracle, split, pendant):
    md, ref, data = _case(oracle, ("irregular", 65), lambda: cases.workload_doc(query_workload("irregular"), 65, seed=65))
    Q = cases.queries(md, data, seed=65)
    user = list(range(len(md["edges"])))
    mixsens_cases.setup_engine(eng, oracle, md)
    for generic in (0, 1):
        eng.set_option(E_.OPT_FORCE_GENERIC, generic)
        try:
            got, sums = eng.place_ll(q_codes=Q, edges=cases.csr_edges(md, user), split=split, pendant_rate=pendant)
        finally:
            eng.set_option(E_.OPT_FORCE_GENERIC, 0)
        # with pendant rate 0 the query's state is the new node's, and with split 1 that node is b: where a leaf b carries
        # another state the site is impossible and the oracle says -inf too; the sums of every other row are compared
        _check_rows(ref, Q, user, got, sums, None, split, pendant)


# ---------------------------------------------------------------- chunking, order, repetition, long lists
def _full(eng, oracle, name, S, Q=None):
    md, ref, data = _case(oracle, (name, S), lambda: cases.workload_doc(query_workload(name), S, seed=S))
    mixsens_cases.setup_engine(eng, oracle, md)
    Q = cases.queries(md, data, seed=S) if Q is None else Q
    return md, Q


def test_chunked_call_gives_the_same_bits(eng, oracle):
    for name in ("irregular", "balanced64"):                    # the k = 4 kernel and the generic one
        md, Q = _full(eng, oracle, name, 257)
        wt = cases.six_decade_weights(257, 9)
        eng.set_site_weights(wt)
        try:
            whole, whole_sums = eng.place_ll(q_codes=Q, split=SPLIT, pendant_rate=PENDANT)
            eng.set_option(E_.OPT_SITE_CHUNK, 100)
            parts, part_sums = eng.place_ll(q_codes=Q, split=SPLIT, pendant_rate=PENDANT)
        finally:
            eng.set_option(E_.OPT_SITE_CHUNK, 0)
            eng.set_site_weights(None)
        assert np.array_equal(whole, parts)
        # the sums of three chunks are added in another order: same values to the sums bar
        assert np.all(np.abs(_dd(whole_sums) - _dd(part_sums)) <= cases.SUM_TOL * np.abs(_dd(whole_sums)))


def test_order_and_repetition(eng, oracle):
    for name in ("balanced32", "irregular", "balanced64"):
        md, Q = _full(eng, oracle, name, 65)
        E = len(md["edges"])
        base, base_sums = eng.place_ll(q_codes=Q, split=SPLIT, pendant_rate=PENDANT)
        assert base.shape == (3, E, 65)
        rng = np.random.default_rng(5)
        pick = np.concatenate([rng.permutation(E)[: E // 2], [3, 3, 0]]).astype(np.int32)      # half of the list, shuffled, repeats
        got, sums = eng.place_ll(q_codes=Q, edges=pick, split=SPLIT, pendant_rate=PENDANT)
        assert np.array_equal(got, base[:, pick]) and np.array_equal(sums, base_sums[:, pick])
        one, one_sum = eng.place_ll(q_codes=Q[1:2], edges=[7], split=SPLIT, pendant_rate=PENDANT)   # one row alone
        assert np.array_equal(one[0, 0], base[1, 7]) and np.array_equal(one_sum[0, 0], base_sums[1, 7])


def test_long_list_runs_in_passes(eng, oracle):
    """3 queries x 200 rows, more than one pass takes (256): the later passes read the stored forward vectors"""
    for name in ("balanced32", "balanced64"):
        md, Q = _full(eng, oracle, name, 65)
        E = len(md["edges"])
        base, base_sums = eng.place_ll(q_codes=Q, split=SPLIT, pendant_rate=PENDANT)
        pick = (np.arange(200) % E).astype(np.int32)
        got, sums = eng.place_ll(q_codes=Q, edges=pick, split=SPLIT, pendant_rate=PENDANT)
        assert got.shape == (3, 200, 65)
        assert np.array_equal(got, base[:, pick]) and np.array_equal(sums, base_sums[:, pick])


def test_many_queries_on_two_edges(eng, oracle):
    """300 queries: one edge spans two passes"""
    md, ref, data = _case(oracle, ("irregular", 65), lambda: cases.workload_doc(query_workload("irregular"), 65, seed=65))
    mixsens_cases.setup_engine(eng, oracle, md)
    rng = np.random.default_rng(11)
    Q = rng.integers(0, len(md["character_definitions"]), (300, 65)).astype(np.uint8)
    user = [9, 16]
    for generic in (0, 1):
        eng.set_option(E_.OPT_FORCE_GENERIC, generic)
        try:
            got, sums = eng.place_ll(q_codes=Q, edges=cases.csr_edges(md, user), split=SPLIT, pendant_rate=PENDANT)
            few, few_sums = eng.place_ll(q_codes=Q[[0, 255, 256, 299]], edges=cases.csr_edges(md, user), split=SPLIT, pendant_rate=PENDANT)
        finally:
            eng.set_option(E_.OPT_FORCE_GENERIC, 0)
        assert np.array_equal(got[[0, 255, 256, 299]], few) and np.array_equal(sums[[0, 255, 256, 299]], few_sums)
        _check_rows(ref, Q[[0, 255, 256, 299]], user, few, few_sums, None)


# ---------------------------------------------------------------- against the engine itself
def test_against_ll_of_a_fresh_engine_on_the_augmented_tree(eng):
    wl = query_workload("irregular")
    S = 100003
    codes = np.ascontiguousarray(np.tile(wl.random_codes(257, seed=3), (1, S // 257 + 1))[:, :S])
    wl.setup_engine(eng)
    eng.set_patterns_codes(codes, wl.defs)
    rng = np.random.default_rng(4)
    q = np.ascontiguousarray(np.tile(rng.integers(0, wl.nchar, 257), S // 257 + 1)[:S].astype(np.uint8))
    user = [0, 10, 16]
    order = synth.csr_from_edges(wl.edges)[3]
    got, sums = eng.place_ll(q_codes=q[None, :], edges=[order[e] for e in user], split=SPLIT, pendant_rate=PENDANT)
    assert eng.info(E_.INFO_PLACE_KERNEL) == 1
    k0 = wl.prepare()
    mode, rw = wl.root_engine()
    miss = next(c for c in range(wl.nchar) if np.all(wl.defs[c] == 1.0))
    for i, e in enumerate(user):
        u, b = wl.edges[e]
        edges2 = [list(x) for x in wl.edges]
        edges2[e] = [u, wl.N]
        edges2 += [[wl.N, b], [wl.N, wl.N + 1]]
        rates2 = list(wl.edge_rates) + [(1.0 - SPLIT) * wl.edge_rates[e], PENDANT]
        rates2[e] = SPLIT * wl.edge_rates[e]
        indptr, indices, preorder, order2 = synth.csr_from_edges(edges2)
        rates = np.zeros(len(edges2))
        rates[order2] = rates2
        codes2 = np.ascontiguousarray(np.vstack([codes, np.full((1, S), miss, dtype=codes.dtype), q[None, :]]))
        fresh = Engine(0)
        try:
            fresh.set_tree(indptr, indices, preorder)
            fresh.set_model(k0["Qn"], rates, k0["cat_rates"], k0["cat_prior"], mode, rw, Qn_lo=k0["Qn_lo"])
            fresh.set_patterns_codes(codes2, wl.defs)
            want, (hi, lo) = fresh.ll()
        finally:
            fresh.close()
        assert cases.site_err(got[0, i], want) <= cases.SITE_TOL
        assert abs(float(_dd(sums)[0, i]) - (hi + lo)) <= cases.SUM_TOL * abs(hi + lo)


# ---------------------------------------------------------------- zero likelihood
def test_zero_likelihood(eng, oracle):
    """onto the rate-0 edge 20 -> 21 with pendant rate 0 the query's state is the state of 20: at site 0 node 20 carries
    another state"""
    wl = query_workload("irregular")
    md = cases.workload_doc(wl, 8, seed=8)
    edges = md["edges"]
    e = edges.index([20, 21])
    assert md["edge_rate_coefficients"][e] == 0.0
    data = [list(row) for row in md["character_data"]]
    miss = cases.missing_code(md)[1]
    for row in data:
        row[20] = miss
    data[0][20] = 0
    md = dict(md, character_data=data)
    q = np.full(8, miss, dtype=np.uint8)
    q[0] = 1
    q[3] = 2
    ref = cases.Reference(oracle, md)
    want = ref.place(e, q, 0.5, 0.0)
    assert np.isneginf(want[0]) and np.all(np.isfinite(want[1:])) and np.all(np.isfinite(ref.current()))
    mixsens_cases.setup_engine(eng, oracle, md)
    csr = cases.csr_edges(md, [e])
    for generic in (0, 1):
        eng.set_option(E_.OPT_FORCE_GENERIC, generic)
        try:
            got, sums = eng.place_ll(q_codes=q[None, :], edges=csr, split=0.5, pendant_rate=0.0)
            assert eng.info(E_.INFO_PLACE_KERNEL) == 1 + generic
            assert np.isneginf(got[0, 0, 0]) and cases.site_err(got[0, 0], want) <= cases.SITE_TOL
            assert not np.isfinite(sums[0, 0, 0] + sums[0, 0, 1])     # as plk_ll: a site of likelihood 0 and weight 1
            wt = np.linspace(0.5, 2.0, 8)
            wt[0] = 0.0                                         # weight exactly 0: the site adds nothing
            eng.set_site_weights(wt)
            _, sums = eng.place_ll(q_codes=q[None, :], edges=csr, split=0.5, pendant_rate=0.0)
            ws = cases.weighted_sum(want, wt)
            assert abs(_dd(sums)[0, 0] - ws) <= cases.SUM_TOL * abs(ws)
        finally:
            eng.set_site_weights(None)
            eng.set_option(E_.OPT_FORCE_GENERIC, 0)


# ---------------------------------------------------------------- refusals
def test_refusals(eng, oracle):
    md, Q = _full(eng, oracle, "irregular", 65)
    E = len(md["edges"])
    good = dict(q_codes=Q, split=SPLIT, pendant_rate=PENDANT)
    base, base_sums = eng.place_ll(**good)
    dense = _dense_queries(md, Q)
    nan_dense, neg_dense = dense.copy(), dense.copy()
    nan_dense[1, 2, 5] = np.nan
    neg_dense[0, 0, 0] = -0.5
    bad_code = Q.copy()
    bad_code[2, 40] = len(md["character_definitions"])
    for kw, word in ((dict(good, q_codes=None), "q_codes"), (dict(good, q_dense=dense), "q_codes"), (dict(good, q_codes=None, q_dense=dense), "q_dense"),
                     (dict(good, q_codes=bad_code), "q_codes"), (dict(good, edges=[0, E]), "edges[1]"), (dict(good, edges=[-1]), "edges[0]"),
                     (dict(good, split=-0.1), "split"), (dict(good, split=1.5), "split"), (dict(good, split=np.nan), "split"),
                     (dict(good, pendant_rate=-1.0), "pendant_rate"), (dict(good, pendant_rate=np.inf), "pendant_rate"),
                     (dict(good, pendant_rate=np.nan), "pendant_rate"), (dict(good, pendant_rate=1e300), "pendant edge")):
        with pytest.raises(EngineError) as ei:
            eng.place_ll(**kw)
        assert ei.value.code == E_.E_ARG and word in str(ei.value), (word, str(ei.value))
    none, no_sums = eng.place_ll(per_site=False, want_sums=False, **good)       # nothing asked for: checked, nothing runs
    assert none is None and no_sums is None
    with pytest.raises(EngineError):
        eng.place_ll(per_site=False, want_sums=False, **dict(good, split=2.0))
    again, again_sums = eng.place_ll(**good)                    # the engine stays usable and gives the same bits
    assert np.array_equal(base, again) and np.array_equal(base_sums, again_sums)
    # dense patterns: the other form is the wrong one; entries must be finite and not negative
    eng.set_patterns_dense(np.ascontiguousarray(np.transpose(oracle.parse_model(md).B, (1, 2, 0))))
    dbase, _ = eng.place_ll(q_dense=dense, split=SPLIT, pendant_rate=PENDANT)
    for kw, word in ((dict(good), "q_dense"), (dict(good, q_codes=None, q_dense=nan_dense), "not finite"),
                     (dict(good, q_codes=None, q_dense=neg_dense), "negative")):
        with pytest.raises(EngineError) as ei:
            eng.place_ll(**kw)
        assert ei.value.code == E_.E_ARG and word in str(ei.value), (word, str(ei.value))
    dagain, _ = eng.place_ll(q_dense=dense, split=SPLIT, pendant_rate=PENDANT)
    assert np.array_equal(dbase, dagain)
    # nothing set yet
    fresh = Engine(0)
    try:
        with pytest.raises(EngineError) as ei:
            fresh.place_ll(**good)
        assert ei.value.code == E_.E_ARG and "must be set" in str(ei.value)
    finally:
        fresh.close()


# ---------------------------------------------------------------- history
def _history_steps(Q, new_rates, old_rates, order):
    def flat(*xs):
        return tuple(np.asarray(x) for x in xs if x is not None)
    place = ("place", lambda e: flat(*e.place_ll(q_codes=Q, split=SPLIT, pendant_rate=PENDANT)))
    steps = {"ll": ("ll", lambda e: flat(e.ll()[0], e.ll()[1])), "deriv": ("deriv", lambda e: flat(*e.deriv())),
             "nni": ("nni", lambda e: flat(*e.nni_ll())),
             "rates": ("update_edge_rates", lambda e: (e.update_edge_rates(new_rates), ())[1]),
             "back": ("update_edge_rates_back", lambda e: (e.update_edge_rates(old_rates), ())[1])}
    out = []
    for name in order:
        out += [steps[name], place]
    return [place] + out


@pytest.mark.parametrize("order", [("ll", "deriv", "nni", "rates", "back"), ("nni", "rates", "ll", "back", "deriv"),
                                   ("rates", "deriv", "back", "nni", "ll")], ids=["a", "b", "c"])
def test_history(order):
    """placement between ll, deriv, nni and a rate change and back on one engine: every result bit for bit what a fresh
    engine brought to the same state gives"""
    wl = query_workload("balanced32")
    S = 300
    codes = wl.random_codes(S, seed=2)
    rng = np.random.default_rng(6)
    Q = rng.integers(0, wl.nchar, (2, S)).astype(np.uint8)
    old_rates = np.asarray(wl.edge_rates_csr, dtype=float)
    new_rates = old_rates * np.linspace(0.7, 1.4, wl.E)
    steps = _history_steps(Q, new_rates, old_rates, order)
    wt = cases.six_decade_weights(S, 21)

    def fresh(updated):
        e = Engine(0)
        wl.setup_engine(e)
        e.set_patterns_codes(codes, wl.defs)
        e.set_site_weights(wt)
        if updated:
            e.update_edge_rates(new_rates)
        return e

    one = fresh(False)
    try:
        seq = [call(one) for _, call in steps]
    finally:
        one.close()
    updated = False
    for i, (name, call) in enumerate(steps):
        if name.startswith("update_edge_rates"):
            updated = name == "update_edge_rates"
            continue
        e = fresh(updated)
        try:
            alone = call(e)
        finally:
            e.close()
        assert len(alone) == len(seq[i]) > 0
        for x, y in zip(alone, seq[i]):
            assert np.array_equal(x, y, equal_nan=True), (i, name)


# ---------------------------------------------------------------- JSON, CLI, Python
def _cli(doc, env=None):
    p = subprocess.run([os.path.join(ROOT, "phyly_amd", "csrc", "arbplf-place")], input=json.dumps(doc).encode(),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **(env or {})))
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def _three_ways(doc):
    import arbplf
    from phyly_amd import arbplf as string_api
    texts = [arbplf.arbplf_place(json.dumps(doc)), string_api._call("arbplf_place", json.dumps(doc))]
    rc, text, err = _cli(doc)
    assert rc == 0, err
    texts.append(text.strip())
    assert texts[0] == texts[1] == texts[2]                     # byte for byte
    return json.loads(texts[0])


def _felsenstein():
    base = load_json(FELSENSTEIN)
    md = base["model_and_data"]
    S, N = len(md["probability_array"]), len(md["edges"]) + 1
    assert S == 1 and N == 8
    # more sites: the document's site with the leaf states rotated
    rows = [md["probability_array"][0]]
    for s in range(1, 5):
        rows.append([row[s % 4:] + row[:s % 4] for row in rows[0]])
    md = dict(md, probability_array=rows)
    queries = [[[1.0, 0.0, 0.0, 0.0], [0.25, 1.0, 0.5, 0.0]], [[0.0, 0.0, 1.0, 0.0], [1.0, 1.0, 1.0, 1.0]], [[0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0]],
               [[1.0, 1.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0]], [[0.0, 0.0, 0.0, 1.0], [0.5, 0.5, 0.5, 0.5]]]
    return {"model_and_data": md}, queries


@pytest.mark.parametrize("reduction", [None, {"aggregation": "sum"}, {"selection": [3, 0, 3], "aggregation": [0.5, -2.0, 1.25]}], ids=["sites", "sum", "weighted"])
@pytest.mark.parametrize("listed", [False, True])
def test_json_cli_python(oracle, reduction, listed):
    base, queries = _felsenstein()
    md = base["model_and_data"]
    E, S = len(md["edges"]), len(queries)
    edges = [4, 0, 6, 4] if listed else list(range(E))          # not in document order, with a repeat
    doc = dict(base, placement={"probability_array": queries, "pendant_rate": 0.2, "split": 0.25})
    if listed:
        doc["placement"]["edges"] = edges
    if reduction:
        doc["site_reduction"] = reduction
    out = _three_ways(doc)
    ref = cases.Reference(oracle, md)
    want = {(qi, e): ref.place(e, [queries[s][qi] for s in range(S)], 0.25, 0.2) for qi in range(2) for e in set(edges)}
    rows = out["data"]
    if reduction is None:
        assert out["columns"] == ["site", "query", "edge", "value"]
        assert [r[:3] for r in rows] == [[s, qi, e] for s in range(S) for qi in range(2) for e in edges]
        for s, qi, e, v in rows:
            assert abs(v - want[qi, e][s]) <= cases.SITE_TOL * max(1.0, abs(v))
    else:
        assert out["columns"] == ["query", "edge", "value"]
        assert [r[:2] for r in rows] == [[qi, e] for qi in range(2) for e in edges]
        sel = reduction.get("selection", list(range(S)))
        wts = reduction["aggregation"] if isinstance(reduction["aggregation"], list) else [1.0] * len(sel)
        for qi, e, v in rows:
            ws = float(sum(cases.LD(w) * cases.LD(want[qi, e][s]) for w, s in zip(wts, sel)))
            assert abs(v - ws) <= cases.SUM_TOL * max(1.0, abs(ws))


def test_json_default_split_is_a_half(oracle):
    base, queries = _felsenstein()
    doc = dict(base, placement={"probability_array": queries, "pendant_rate": 0.2, "edges": [2]})
    out = _three_ways(doc)
    ref = cases.Reference(oracle, base["model_and_data"])
    want = ref.place(2, [queries[s][0] for s in range(len(queries))], 0.5, 0.2)
    assert abs(out["data"][0][3] - want[0]) <= cases.SITE_TOL * max(1.0, abs(want[0]))


def test_patterns_are_keyed_on_the_queries_too(oracle):
    """40 sites of three joint patterns: sites of pattern 0 and 1 agree on every node of the tree and differ in one query"""
    md1 = mixsens_cases.five_taxon_doc(2, 4, seed=9)
    tree_rows = [md1["character_data"][0], md1["character_data"][0], md1["character_data"][1]]
    query_rows = [[0, 2], [0, 3], [1, 4]]
    which = [s % 3 for s in range(40)]
    md = dict(md1, character_data=[tree_rows[w] for w in which])
    placement = {"character_data": [query_rows[w] for w in which], "pendant_rate": 0.15, "split": 0.4, "edges": [5, 1]}
    ref = cases.Reference(oracle, md)
    want = {(qi, e): ref.place(e, [query_rows[w][qi] for w in which], 0.4, 0.15) for qi in range(2) for e in (5, 1)}
    out = _three_ways({"model_and_data": md, "placement": placement})
    got = {(s, qi, e): v for s, qi, e, v in out["data"]}
    assert len(got) == 40 * 2 * 2
    for (s, qi, e), v in got.items():
        assert abs(v - want[qi, e][s]) <= cases.SITE_TOL * max(1.0, abs(v))
    assert got[0, 0, 5] == got[1, 0, 5] and got[0, 1, 5] != got[1, 1, 5]       # the same tree columns, another second query
    assert abs(want[1, 5][0] - want[1, 5][1]) > cases.MOVES
    summed = _three_ways({"model_and_data": md, "placement": placement, "site_reduction": {"aggregation": "sum"}})
    for qi, e, v in summed["data"]:
        ws = float(np.sum(np.asarray(want[qi, e], dtype=cases.LD)))
        assert abs(v - ws) <= cases.SUM_TOL * abs(ws)


def test_json_errors():
    import arbplf
    base, queries = _felsenstein()
    for placement, word in (({"probability_array": queries}, "pendant_rate"), ({"probability_array": queries, "pendant_rate": 0.2, "edges": [7]}, "edges"),
                            ({"character_data": [[0, 1]] * 5, "pendant_rate": 0.2}, "probability_array"),
                            ({"probability_array": queries, "pendant_rate": 0.2, "split": 1.5}, "split")):
        doc = dict(base, placement=placement)
        with pytest.raises(RuntimeError):
            arbplf.arbplf_place(json.dumps(doc))
        rc, text, err = _cli(doc)
        assert rc != 0 and text == "" and word in err


def test_cli_without_a_gpu_has_no_fallback():
    base, queries = _felsenstein()
    doc = dict(base, placement={"probability_array": queries, "pendant_rate": 0.2})
    rc, text, err = _cli(doc, env={"HIP_VISIBLE_DEVICES": "", "ROCR_VISIBLE_DEVICES": ""})
    assert rc == 255 and text == "" and "no CPU fallback" in err


# ---------------------------------------------------------------- groups
def test_group_of_two_engines(oracle):
    md, ref, data = _case(oracle, ("irregular", 257), lambda: cases.workload_doc(query_workload("irregular"), 257, seed=257))
    m = oracle.parse_model(md)
    k0 = mixsens_cases.product_k0(m)
    Q = cases.queries(md, data, seed=257)
    codes = np.ascontiguousarray(data.astype(np.uint8).T)
    defs = np.asarray(md["character_definitions"], dtype=float)
    rw = np.asarray(m.root_custom, dtype=float)
    wt = cases.six_decade_weights(257, 5)
    E = m.E
    lib = E_.load_library()
    import ctypes
    vp, ci, cl, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_double
    lib.plk_group_create.argtypes = [ctypes.POINTER(vp), ci, vp]
    lib.plk_group_destroy.argtypes = [vp]
    lib.plk_group_set_tree.argtypes = [vp, ci, vp, vp, vp]
    lib.plk_group_set_model.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp, ci, vp]
    lib.plk_group_set_patterns_codes.argtypes = [vp, cl, vp, ci, vp]
    lib.plk_group_set_site_weights.argtypes = [vp, vp]
    lib.plk_group_place_ll.argtypes = [vp, ci, vp, vp, ci, vp, cd, cd, vp, vp]
    lib.plk_group_last_error.argtypes = [vp]
    lib.plk_group_last_error.restype = ctypes.c_char_p
    results = []
    for devs in ([0], [0, 0]):
        g = vp()
        dev = np.array(devs, dtype=np.int32)
        assert lib.plk_group_create(ctypes.byref(g), len(devs), E_._ptr(dev)) == 0
        try:
            def ok(rc):
                assert rc == 0, lib.plk_group_last_error(g)
            ok(lib.plk_group_set_tree(g, m.N, E_._ptr(m.indptr), E_._ptr(m.indices), E_._ptr(m.preorder)))
            er = np.ascontiguousarray(m.edge_rates_csr, dtype=float)
            ok(lib.plk_group_set_model(g, m.k, k0["C"], E_._ptr(k0["Qn"]), E_._ptr(k0["Qn_lo"]), E_._ptr(er), E_._ptr(k0["cat_rates"]),
                                       E_._ptr(k0["cat_prior"]), m.root_mode, E_._ptr(rw)))
            ok(lib.plk_group_set_patterns_codes(g, 257, E_._ptr(codes), len(defs), E_._ptr(defs)))
            ok(lib.plk_group_set_site_weights(g, E_._ptr(wt)))
            out, sums = np.zeros((3, E, 257)), np.zeros((3, E, 2))
            ok(lib.plk_group_place_ll(g, 3, E_._ptr(Q), None, E, None, SPLIT, PENDANT, E_._ptr(out), E_._ptr(sums)))
            results.append((out, sums))
        finally:
            lib.plk_group_destroy(g)
    (one, one_sums), (two, two_sums) = results
    assert np.array_equal(one, two)
    assert np.all(np.abs(_dd(one_sums) - _dd(two_sums)) <= cases.SUM_TOL * np.abs(_dd(one_sums)))
    user_of_csr = np.argsort(synth.csr_from_edges(md["edges"])[3])
    _check_rows(ref, Q[:1], [int(user_of_csr[3])], one[:1, 3:4], one_sums[:1, 3:4], wt)
