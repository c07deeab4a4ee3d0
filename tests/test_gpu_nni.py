"""GPU: plk_nni_ll / arbplf-nni against the oracle's ll of the swapped tree (tests/nni_cases.py rewrites the two parents in
the model document).  Bars: per site |d| <= 1e-12 max(1, |ll'|); sums within 1e-12 of the long double host sum of the
reference values, the bar tests/test_gpu_ll.py holds plk_ll sums to.

The swap kernels run on a grid over the site chunk (plk_nni.h says why), so there is no second batch pass to test; the
chunked call below covers a grid that starts inside the pattern rows."""
import json
import os
import subprocess

import numpy as np
import pytest

import mixsens_cases
import nni_cases as cases
from helpers import GOLDEN, K4_MODELS, QUERY_MODEL, family_workload, load_json, query_workload
from phyly_amd import engine as E_, synth
from phyly_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FELSENSTEIN = os.path.join(GOLDEN, "examples", "Felsenstein.2004.fig.16.4", "ll", "in.json")
_refs = {}


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _case(oracle, key, build):
    """(md, Reference, canonical swaps in user indices in the order of the canonical CSR list), built once per module"""
    if key not in _refs:
        md = build()
        ref = cases.Reference(oracle, md)
        canon = cases.csr_to_user(md["edges"], E_.nni_swaps(ref.m.indptr, ref.m.indices))
        _refs[key] = (md, ref, canon)
    return _refs[key]


def _dd(sums):
    return np.asarray(sums[:, 0], dtype=cases.LD) + np.asarray(sums[:, 1], dtype=cases.LD)


def _check_rows(ref, pairs, got, sums, wt, skip=()):
    worst = 0.0
    for i, (a, b) in enumerate(pairs):
        if (a, b) in skip:
            continue
        want = ref.swap(a, b)
        err = cases.site_err(got[i], want)
        worst = max(worst, err)
        assert err <= cases.SITE_TOL, (a, b, err)
        if sums is not None:
            ws = cases.weighted_sum(want, wt)
            assert abs(_dd(sums)[i] - ws) <= cases.SUM_TOL * abs(ws), (a, b, float(_dd(sums)[i]), float(ws))
    return worst


# stack slots of each model's tree (tests/test_gpu_k4_variants.py SHAPE; balanced64g3 is the balanced64 tree) and the
# k_down_fused4<D> that goes with them: D = 4 up to 4 slots, 8 up to 8
SLOTS = {"irregular": 1, "balanced32": 4, "balanced64": 5, "wide": 1, QUERY_MODEL: 5}
DOWN4 = {"irregular": 4, "balanced32": 4, "balanced64": 8, "wide": 4, QUERY_MODEL: 8}


# ---------------------------------------------------------------- the k = 4 models
@pytest.mark.parametrize("S", [1, 65, 257])
@pytest.mark.parametrize("name", list(K4_MODELS) + [QUERY_MODEL])
def test_k4_models(eng, oracle, name, S):
    md, ref, canon = _case(oracle, (name, S), lambda: cases.workload_doc(query_workload(name), S, seed=S))
    skip = cases.STILL_SWAPS.get(name, ())
    assert len(canon) > 20
    C = ref.w["C"]
    wt = cases.six_decade_weights(S, 3 + S)
    for layout in ("compact", "generic", "dense"):
        mixsens_cases.setup_engine(eng, oracle, md)
        if layout == "dense":
            eng.set_patterns_dense(np.ascontiguousarray(np.transpose(ref.m.B, (1, 2, 0))))
        eng.set_option(E_.OPT_FORCE_GENERIC, 1 if layout == "generic" else 0)
        try:
            before = eng.info(E_.INFO_DOWN4_KERNEL)
            got, sums = eng.nni_ll()
            k4 = layout == "compact" and C <= 4
            assert eng.info(E_.INFO_NNI_KERNEL) == (1 if k4 else 2), (name, layout)
            slots = eng.info(E_.INFO_STACK_SLOTS)
            assert slots == SLOTS[name]
            assert eng.info(E_.INFO_DOWN4_KERNEL) == (DOWN4[name] if k4 else before)      # latched by the k = 4 passes only
            if name == "balanced64":
                assert C == 5 and eng.info(E_.INFO_NNI_KERNEL) == 2
            if name == QUERY_MODEL and layout == "compact":
                assert slots == 5 and eng.info(E_.INFO_NNI_KERNEL) == 1 and eng.info(E_.INFO_DOWN4_KERNEL) == 8
            worst = _check_rows(ref, canon, got, sums, None, skip)
            eng.set_site_weights(wt)
            got_w, sums_w = eng.nni_ll()
            assert np.array_equal(got, got_w)                   # weights touch the sums only
            _check_rows(ref, canon, got_w, sums_w, wt, skip)
            print("%s S=%d %s: %d swaps, worst site error %.2e" % (name, S, layout, len(canon), worst))
        finally:
            eng.set_site_weights(None)
            eng.set_option(E_.OPT_FORCE_GENERIC, 0)


# ---------------------------------------------------------------- other state counts
@pytest.mark.parametrize("k", [2, 5, 13, 27, 48])
def test_family_models(eng, oracle, k):
    md, ref, _ = _case(oracle, ("family", k), lambda: cases.workload_doc(family_workload(k), 65, seed=k))
    edges = md["edges"]
    pairs = cases.sample_swaps(edges, 16, seed=k)
    into, parents = cases.in_edges(edges), {p for p, _ in edges}
    assert any(edges[b][0] not in into for _, b in pairs)                 # one under the root
    assert any(edges[a][1] not in parents for a, _ in pairs)              # a leaf c
    assert any(edges[b][1] not in parents for _, b in pairs)              # a leaf s
    mixsens_cases.setup_engine(eng, oracle, md)
    wt = cases.six_decade_weights(65, k)
    eng.set_site_weights(wt)
    try:
        got, sums = eng.nni_ll(cases.user_to_csr(edges, pairs))
    finally:
        eng.set_site_weights(None)
    assert eng.info(E_.INFO_NNI_KERNEL) == 2
    print("k=%d: %d swaps, worst site error %.2e" % (k, len(pairs), _check_rows(ref, pairs, got, sums, wt)))


# ---------------------------------------------------------------- carried-over scale factors
@pytest.mark.parametrize("k", [4, 13])
def test_ladder_of_200_leaves(eng, oracle, k):
    """edge rates near 1 and observation rows scaled by 1e-4: every site likelihood is far below 2^-1022, and a swap moves a
    subtree past the rescaled nodes of the ladder"""
    md, ref, _ = _case(oracle, ("ladder", k), lambda: cases.ladder_doc(200, 33, seed=40 + k, k=k, C=2, leaf_scale=1e-4))
    assert np.max(ref.current()) < -1022 * np.log(2.0) - 100
    pairs = cases.sample_swaps(md["edges"], 16, seed=k, spread=True)
    mixsens_cases.setup_engine(eng, oracle, md)
    got, sums = eng.nni_ll(cases.user_to_csr(md["edges"], pairs))
    assert eng.info(E_.INFO_NNI_KERNEL) == (1 if k == 4 else 2)
    assert np.all(np.isfinite(got))
    print("ladder k=%d: worst site error %.2e" % (k, _check_rows(ref, pairs, got, sums, None)))


# ---------------------------------------------------------------- chunking, order, repetition
def test_chunked_call_gives_the_same_bits(eng, oracle):
    for name in ("irregular", "balanced64"):                    # the k = 4 kernel and the generic one
        md, ref, canon = _case(oracle, (name, 257), lambda: cases.workload_doc(query_workload(name), 257, seed=257))
        mixsens_cases.setup_engine(eng, oracle, md)
        wt = cases.six_decade_weights(257, 9)
        eng.set_site_weights(wt)
        try:
            whole, whole_sums = eng.nni_ll()
            eng.set_option(E_.OPT_SITE_CHUNK, 100)
            parts, part_sums = eng.nni_ll()
        finally:
            eng.set_option(E_.OPT_SITE_CHUNK, 0)
            eng.set_site_weights(None)
        assert np.array_equal(whole, parts)
        # the sums of three chunks are added in another order: same values to the sums bar
        assert np.all(np.abs(_dd(whole_sums) - _dd(part_sums)) <= cases.SUM_TOL * np.abs(_dd(whole_sums)))


def test_order_and_repetition(eng, oracle):
    for name in ("balanced32", "irregular", "balanced64"):      # records of two swaps, of one, the generic kernel
        md, ref, canon = _case(oracle, (name, 65), lambda: cases.workload_doc(query_workload(name), 65, seed=65))
        mixsens_cases.setup_engine(eng, oracle, md)
        csr = E_.nni_swaps(ref.m.indptr, ref.m.indices)
        base, base_sums = eng.nni_ll()
        rng = np.random.default_rng(5)
        pick = np.concatenate([rng.permutation(len(csr))[: len(csr) // 2], [3, 3, 0]])       # half of the list, shuffled, repeats
        got, sums = eng.nni_ll(csr[pick])
        assert np.array_equal(got, base[pick]) and np.array_equal(sums, base_sums[pick])
        one, _ = eng.nni_ll(csr[7:8])                           # one swap of an edge whose two swaps share a record
        assert np.array_equal(one[0], base[7])


def test_long_list_runs_in_groups(eng, oracle):
    """more swaps than one up pass takes (256): the later groups read the stored forward vectors"""
    md, ref, canon = _case(oracle, ("balanced32", 65), lambda: cases.workload_doc(query_workload("balanced32"), 65, seed=65))
    mixsens_cases.setup_engine(eng, oracle, md)
    csr = E_.nni_swaps(ref.m.indptr, ref.m.indices)
    base, base_sums = eng.nni_ll()
    pick = np.arange(600) % len(csr)
    got, sums = eng.nni_ll(csr[pick])
    assert np.array_equal(got, base[pick]) and np.array_equal(sums, base_sums[pick])


# ---------------------------------------------------------------- refusals
def test_pairs_that_are_no_swap_are_refused(eng, oracle):
    md, ref, canon = _case(oracle, ("irregular", 65), lambda: cases.workload_doc(query_workload("irregular"), 65, seed=65))
    edges = md["edges"]
    mixsens_cases.setup_engine(eng, oracle, md)
    base, _ = eng.nni_ll()
    into = cases.in_edges(edges)
    a, b = cases.swaps_user(edges)[5]
    deep = next(e for e, (p, c) in enumerate(edges) if p in into and into[p][1] in into and into[into[p][1]][1] == edges[b][0])
    for pair in ((a, a), (a, into[edges[a][0]][0]), (deep, b), (b, a)):
        assert cases.why_no_swap(edges, *pair)
        bad = np.concatenate([cases.user_to_csr(edges, canon[:2]), cases.user_to_csr(edges, [pair])])
        with pytest.raises(EngineError) as ei:
            eng.nni_ll(bad)
        assert ei.value.code == E_.E_ARG and "pair 2 " in str(ei.value) and "no swap" in str(ei.value)
    for bad in ([[0, len(edges)]], [[-1, 0]]):
        with pytest.raises(EngineError) as ei:
            eng.nni_ll(np.array(bad, dtype=np.int32))
        assert ei.value.code == E_.E_ARG and "out of range" in str(ei.value)
    again, _ = eng.nni_ll()                                     # the engine stays usable
    assert np.array_equal(base, again)


# ---------------------------------------------------------------- against the engine itself
def test_against_ll_of_a_fresh_engine_on_the_swapped_tree(eng):
    wl = query_workload("irregular")
    S = 100003
    codes = np.ascontiguousarray(np.tile(wl.random_codes(257, seed=3), (1, S // 257 + 1))[:, :S])
    wl.setup_engine(eng)
    eng.set_patterns_codes(codes, wl.defs)
    pairs = [cases.swaps_user(wl.edges)[i] for i in (0, 11, 23)]
    got, sums = eng.nni_ll(cases.user_to_csr(wl.edges, pairs))
    assert eng.info(E_.INFO_NNI_KERNEL) == 1
    k0 = wl.prepare()
    mode, rw = wl.root_engine()
    for i, (a, b) in enumerate(pairs):
        edges2 = cases.swap_edges(wl.edges, a, b)
        indptr, indices, preorder, order = synth.csr_from_edges(edges2)
        rates = np.zeros(wl.E)
        rates[order] = wl.edge_rates
        fresh = Engine(0)
        try:
            fresh.set_tree(indptr, indices, preorder)
            fresh.set_model(k0["Qn"], rates, k0["cat_rates"], k0["cat_prior"], mode, rw, Qn_lo=k0["Qn_lo"])
            fresh.set_patterns_codes(codes, wl.defs)
            want, (hi, lo) = fresh.ll()
        finally:
            fresh.close()
        assert cases.site_err(got[i], want) <= cases.SITE_TOL
        assert abs(float(_dd(sums)[i]) - (hi + lo)) <= cases.SUM_TOL * abs(hi + lo)


# ---------------------------------------------------------------- zero likelihood
def test_zero_likelihood(eng, oracle):
    """site 0 is impossible under the current tree (different states at 20 and at its child 21 across the rate-0 edge) and
    possible once 21 hangs from 19; site 1 (states at 19 and 21, none at 20) is impossible only then"""
    wl = query_workload("irregular")
    md = cases.workload_doc(wl, 8, seed=8)
    edges = md["edges"]
    a, b = edges.index([20, 21]), edges.index([19, 8])
    assert md["edge_rate_coefficients"][a] == 0.0 and cases.why_no_swap(edges, a, b) is None
    data = [list(row) for row in md["character_data"]]
    data[0][20], data[0][21] = 0, 1
    data[1][19], data[1][21], data[1][20] = 0, 1, 4
    md = dict(md, character_data=data)
    ref = cases.Reference(oracle, md)
    cur, want = ref.current(), ref.swap(a, b)
    assert np.isneginf(cur[0]) and np.isfinite(want[0]) and np.isfinite(cur[1]) and np.isneginf(want[1])
    assert np.all(np.isfinite(want[2:]))
    mixsens_cases.setup_engine(eng, oracle, md)
    pair = cases.user_to_csr(edges, [(a, b)])
    for generic in (0, 1):
        eng.set_option(E_.OPT_FORCE_GENERIC, generic)
        try:
            ll, _ = eng.ll()
            assert np.isneginf(ll[0]) and np.isfinite(ll[1])
            got, sums = eng.nni_ll(pair)
            assert eng.info(E_.INFO_NNI_KERNEL) == 1 + generic
            assert cases.site_err(got[0], want) <= cases.SITE_TOL
            assert not np.isfinite(sums[0, 0] + sums[0, 1])     # as plk_ll (below): a site of likelihood 0 and weight 1
            wt = np.linspace(0.5, 2.0, 8)
            wt[1] = 0.0                                         # weight exactly 0: the site adds nothing
            eng.set_site_weights(wt)
            _, sums = eng.nni_ll(pair)
            ws = cases.weighted_sum(want, wt)
            assert abs(_dd(sums)[0] - ws) <= cases.SUM_TOL * abs(ws)
            _, (hi, lo) = eng.ll()                              # plk_ll on the current tree, whose impossible site has weight 0.5
            assert not np.isfinite(hi + lo)
        finally:
            eng.set_site_weights(None)
            eng.set_option(E_.OPT_FORCE_GENERIC, 0)


# ---------------------------------------------------------------- history
def _history_steps(wl, codes, new_rates):
    """(name, call) of every step; a step returns what it computed as a tuple of arrays"""
    def flat(*xs):
        return tuple(np.asarray(x) for x in xs if x is not None)
    return [("ll", lambda e: flat(e.ll()[0], e.ll()[1])),
            ("nni", lambda e: flat(*e.nni_ll())),
            ("deriv", lambda e: flat(*e.deriv())),
            ("nni", lambda e: flat(*e.nni_ll())),
            ("update_edge_rates", lambda e: (e.update_edge_rates(new_rates), ())[1]),
            ("nni", lambda e: flat(*e.nni_ll())),
            ("cat_posterior", lambda e: flat(*e.cat_posterior()[:3]))]


@pytest.mark.parametrize("which", ["k4_streamed", "k20"])
def test_history(which):
    """ll, nni, deriv, nni, update_edge_rates, nni, cat_posterior on one engine: every result bit for bit what a fresh
    engine brought to the same state gives"""
    wl = query_workload("balanced32") if which == "k4_streamed" else family_workload(20)
    S = 300 if which == "k4_streamed" else 65
    codes = wl.random_codes(S, seed=2)
    new_rates = np.asarray(wl.edge_rates_csr) * np.linspace(0.7, 1.4, wl.E)
    steps = _history_steps(wl, codes, new_rates)
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
        if which == "k4_streamed":
            one.ll()
            assert one.info(E_.INFO_LL_FORM) == 1               # the streamed ll kernel is what the history runs between
        seq = [call(one) for _, call in steps]
    finally:
        one.close()
    updated = False
    for i, (name, call) in enumerate(steps):
        if name == "update_edge_rates":
            updated = True
            continue
        e = fresh(updated)
        try:
            alone = call(e)
        finally:
            e.close()
        assert len(alone) == len(seq[i]) > 0
        for x, y in zip(alone, seq[i]):
            assert np.array_equal(x, y, equal_nan=True), (i, name)


# ---------------------------------------------------------------- JSON, CLI, groups
def _oracle_rows(oracle, doc, pairs):
    """[first_edge, second_edge, site values...] from the oracle's arbplf_ll on each rewritten document"""
    rows = []
    for a, b in pairs:
        x = dict(doc, model_and_data=cases.swap_doc(doc["model_and_data"], a, b))
        x.pop("swaps", None)
        out = json.loads(oracle.arbplf_ll(json.dumps(x)))
        rows.append((a, b, out))
    return rows


def _cli(doc, env=None):
    p = subprocess.run([os.path.join(ROOT, "phyly_amd", "csrc", "arbplf-nni")], input=json.dumps(doc).encode(),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **(env or {})))
    return p.returncode, p.stdout.decode(), p.stderr.decode()


@pytest.mark.parametrize("agg", [None, "sum"])
@pytest.mark.parametrize("listed", [False, True])
def test_json_and_cli(oracle, agg, listed):
    import arbplf
    from phyly_amd import arbplf as string_api
    base = load_json(FELSENSTEIN)
    edges = base["model_and_data"]["edges"]
    allsw = cases.swaps_user(edges)
    assert len(allsw) == 2 * 2 + 2 * 1                           # 6 under the root (two other children), 5 under 6 (one)
    pairs = [allsw[3], allsw[0], allsw[3]] if listed else allsw
    doc = dict(base)
    if listed:
        doc["swaps"] = [list(p) for p in pairs]
    if agg:
        doc["site_reduction"] = {"aggregation": agg}
    want = _oracle_rows(oracle, doc, pairs)
    outs = [json.loads(arbplf.arbplf_nni(json.dumps(doc))), json.loads(string_api._call("arbplf_nni", json.dumps(doc)))]
    rc, text, err = _cli(doc)
    assert rc == 0, err
    outs.append(json.loads(text))
    for out in outs:
        assert out["columns"] == (["first_edge", "second_edge", "value"] if agg else ["site", "first_edge", "second_edge", "value"])
        assert out == outs[0]
        rows = out["data"]
        if agg:
            assert [r[:2] for r in rows] == [list(p) for p in pairs]
            for r, (a, b, o) in zip(rows, want):
                assert abs(r[2] - o["data"][0][-1]) <= cases.SITE_TOL * max(1.0, abs(r[2]))
        else:
            assert [r[:3] for r in rows] == [[0, a, b] for a, b in pairs]            # one site, rows in the order of the request
            for r, (a, b, o) in zip(rows, want):
                assert o["data"][0][0] == 0 and abs(r[3] - o["data"][0][-1]) <= cases.SITE_TOL * max(1.0, abs(r[3]))


@pytest.mark.parametrize("swaps,word", [([[0, 0]], "no swap"), ([[3, 2]], "no swap"), ([[2, 3]], "no swap"), ([[5, 0]], "no swap"),
                                        ([[3.0, 0]], "integers"), ([[3, 7]], "out of range"), ([[3]], "pair"), ("all", "array")])
def test_json_errors(swaps, word):
    """the same edge twice; s = v (edge 2 ends at 6, where edge 3 starts); reversed order; two levels apart (edge 5 starts
    at 5, a grandchild of the root); a real number; an index out of range; no pair; no array"""
    import arbplf
    doc = dict(load_json(FELSENSTEIN), swaps=swaps)
    with pytest.raises(RuntimeError):
        arbplf.arbplf_nni(json.dumps(doc))
    rc, text, err = _cli(doc)
    assert rc != 0 and text == "" and word in err


def test_group_of_two_engines(monkeypatch, oracle):
    import arbplf
    wl = query_workload("irregular")
    md = cases.workload_doc(wl, 301, seed=12)
    for agg in (None, {"aggregation": "sum"}):
        doc = {"model_and_data": md, "swaps": [list(p) for p in cases.swaps_user(md["edges"])[::5]]}
        if agg:
            doc["site_reduction"] = agg
        monkeypatch.delenv("ARBPLF_DEVICES", raising=False)
        one = json.loads(arbplf.arbplf_nni(json.dumps(doc)))
        monkeypatch.setenv("ARBPLF_DEVICES", "0,0")
        two = json.loads(arbplf.arbplf_nni(json.dumps(doc)))
        monkeypatch.delenv("ARBPLF_DEVICES", raising=False)
        assert one["columns"] == two["columns"] and len(one["data"]) == len(two["data"]) > 0
        for x, y in zip(one["data"], two["data"]):
            assert x[:-1] == y[:-1]
            if agg is None:
                assert x[-1] == y[-1]
            else:
                assert abs(x[-1] - y[-1]) <= 1e-14 * max(abs(x[-1]), 1e-3)
