"""GPU parity of the expectation queries: arbplf-dwell, arbplf-trans,
arbplf-em-update and the engine entry point behind them (plk_edge_expect), against

  * every golden in/out pair the reference holds for these commands (tests/golden/examples),
  * the binary128 oracle on seeded synthetic workloads and on random small models whose every query is feasible
    (tests/expect_cases.py: 60 per command, all compared), with the documents of likelihood zero in a list of their own,
  * closed forms on a pure-birth path and an absorbing two-state path, and the selection / aggregation / mixture
    algebra of the state and pair axes,
  * size-independent identities at larger sizes: dwell proportions sum to 1 over states,
    and d ll / d edge_rate = E[rate-weighted transitions] - E[rate-weighted exits].

Tolerance: |d| <= 1e-12 * max(|expected|, scale), scale = the largest magnitude in the same
table / site row (as for deriv and marginal)."""
import copy
import glob
import json
import os
import random

import numpy as np
import pytest

import expect_cases as cases
from helpers import GOLDEN, load_json, oracle_model

pytestmark = pytest.mark.gpu
EX = os.path.join(GOLDEN, "examples")


def _pairs(dirs):
    out = []
    for d in dirs:
        for inp in sorted(glob.glob(os.path.join(EX, d, "in*.json"))):
            out.append((inp, os.path.join(os.path.dirname(inp), "out" + os.path.basename(inp)[2:])))
    return out


CASES = [("dwell", p) for p in _pairs(["Felsenstein.2004.fig.16.4/dwell/adenine", "Felsenstein.2004.fig.16.4/dwell/pyrimidines",
                                       "BEAST.MarkovJumps/MarkovRewardsC", "JC.long.branch/dwell"])]
CASES += [("trans", p) for p in _pairs(["Felsenstein.2004.fig.16.4/trans/A.to.C.only", "Felsenstein.2004.fig.16.4/trans/all.types",
                                        "Felsenstein.2004.fig.16.4/trans/transversions.only", "BEAST.MarkovJumps/MarkovJumpsC",
                                        "BEAST.MarkovJumps/MarkovMarginalRate", "JC.long.branch/trans"])]
CASES += [("em_update", p) for p in _pairs(["Felsenstein.2004.fig.16.4/em-update/with.full.data",
                                            "Felsenstein.2004.fig.16.4/em-update/with.leaf.data",
                                            "Felsenstein.2004.fig.16.4/em-update/with.no.data"])]


def _prod(kind):
    import arbplf
    return {"ll": arbplf.arbplf_ll, "deriv": arbplf.arbplf_deriv, "dwell": arbplf.arbplf_dwell,
            "trans": arbplf.arbplf_trans, "em_update": arbplf.arbplf_em_update}[kind]


def _orc(oracle, kind):
    return {"dwell": oracle.arbplf_dwell, "trans": oracle.arbplf_trans, "em_update": oracle.arbplf_em_update}[kind]


def _check_table(got, want, rel=1e-12):
    assert got["columns"] == want["columns"]
    assert len(got["data"]) == len(want["data"])
    scale = max([abs(r[-1]) for r in want["data"]] + [0.0])
    for a, b in zip(got["data"], want["data"]):
        assert a[:-1] == b[:-1]
        assert abs(a[-1] - b[-1]) <= rel * abs(b[-1]) + 1e-14 * scale + 1e-300, (a, b)


@pytest.mark.parametrize("kind,pair", CASES, ids=[os.path.relpath(c[1][0], EX) for c in CASES])
def test_reference_goldens(kind, pair):
    inp, outp = pair
    with open(inp) as f:
        got = json.loads(_prod(kind)(f.read()))
    _check_table(got, load_json(outp))


def test_cli_dwell_trans_em(tmp_path):
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for exe, d in (("arbplf-dwell", "Felsenstein.2004.fig.16.4/dwell/adenine"),
                   ("arbplf-trans", "Felsenstein.2004.fig.16.4/trans/all.types"),
                   ("arbplf-em-update", "Felsenstein.2004.fig.16.4/em-update/with.leaf.data"),
                   ("arbplf-dwell", "JC.long.branch/dwell"), ("arbplf-trans", "JC.long.branch/trans")):
        with open(os.path.join(EX, d, "in.json")) as f:
            r = subprocess.run([os.path.join(root, "phyly_amd", "csrc", exe)], stdin=f, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        _check_table(json.loads(r.stdout), load_json(os.path.join(EX, d, "out.json")))
    r = subprocess.run([os.path.join(root, "phyly_amd", "csrc", "arbplf-em-update")], input='{"model_and_data": {}}',
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and r.stdout == ""


# ------------------------------------------------------------------ engine level
@pytest.fixture(scope="module")
def eng():
    from phyly_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _row_err(got, want):
    scale = np.max(np.abs(want), axis=1, keepdims=True)
    return np.max(np.abs(got - want) / np.maximum(np.abs(want), np.maximum(scale, 1e-300)))


def _directions(w, rng):
    k = w.k
    out = []
    L = np.zeros((k, k)); L[rng.integers(k), rng.integers(k)] = 1.0
    out.append(("unit", L, 0))
    out.append(("diag", np.diag(rng.uniform(-1, 2, k)), 0))
    out.append(("dense", rng.uniform(-1, 1, (k, k)), 1))
    out.append(("offdiag", rng.uniform(0, 1, (k, k)) * (1 - np.eye(k)), 2))
    return out


@pytest.mark.parametrize("cfg,S,nreq", [(2, 200, 98), (3, 120, 198), (4, 24, 12), (5, 8, 2)])
def test_edge_expect_matches_oracle(eng, oracle, cfg, S, nreq):
    """plk_edge_expect (fused k=4 path, MFMA path) against the oracle's Frechet matrices + site evaluator"""
    from phyly_amd import synth
    w = synth.Workload(cfg)
    w.setup_engine(eng)
    codes = w.simulate(S)
    m, ow = oracle_model(oracle, w, codes)
    B = w.defs[codes.T]
    eng.set_patterns_codes(codes, w.defs)
    eng.set_site_weights(None)
    rng = np.random.default_rng(1000 + cfg)
    mask = np.zeros(w.E, dtype=np.int32)
    mask[rng.choice(w.E, size=nreq, replace=False)] = 1
    sel = mask.astype(bool)
    precise = 2 if w.k <= 4 else 1
    for name, L, coef in _directions(w, rng):
        F = oracle.frechet(m, ow, L, 1.0, False, mask, precise=precise)
        want = oracle.site_edge_expect(m, ow, B, F, coef, mask, precise=precise)
        got, sums = eng.edge_expect(L, coef, edge_mask=mask)
        assert _row_err(got[:, sel], want[:, sel]) <= 1e-12, (name, coef)
        assert np.all(got[:, ~sel] == 0.0)
        ref = want.astype(np.longdouble).sum(axis=0).astype(float)
        tot = sums[:, 0] + sums[:, 1]
        assert np.max(np.abs(tot[sel] - ref[sel])) <= 1e-12 * np.max(np.abs(ref[sel])), name


@pytest.mark.parametrize("cfg,S,nL", [(3, 300, 2), (3, 257, 5), (2, 64, 4), (4, 16, 3)])
def test_edge_expect_multi_equals_single_calls(eng, cfg, S, nL):
    """several directions per pass (k = 4: up to four share one down / up pass; more are split; other k: one pass
    each) must give exactly what the single-direction entry point gives"""
    from phyly_amd import synth, engine as E
    w = synth.Workload(cfg)
    w.setup_engine(eng)
    codes = w.random_codes(S, seed=cfg)
    eng.set_patterns_codes(codes, w.defs)
    wts = np.linspace(0.5, 1.5, S)
    eng.set_site_weights(wts)
    rng = np.random.default_rng(5 + nL)
    Ls = rng.uniform(-1, 1, (nL, w.k, w.k))
    mask = (rng.random(w.E) < 0.7).astype(np.int32)
    got, gsum = eng.edge_expect_multi(Ls, E.COEF_PRIOR_RATE_EDGE, edge_mask=mask)
    for m in range(nL):
        one, osum = eng.edge_expect(Ls[m], E.COEF_PRIOR_RATE_EDGE, edge_mask=mask)
        assert np.array_equal(got[:, m, :], one)
        assert np.array_equal(gsum[m], osum)
    eng.set_site_weights(None)


@pytest.mark.parametrize("cfg,nreq", [(3, 198), (4, 6), (5, 1)])
def test_frechet_matrices_match_oracle(eng, oracle, cfg, nreq):
    """the device double-double block exponential against the binary128 one, entry by entry"""
    from phyly_amd import synth, engine as E
    w = synth.Workload(cfg)
    w.setup_engine(eng)
    codes = w.simulate(4)
    m, ow = oracle_model(oracle, w, codes)
    rng = np.random.default_rng(77 + cfg)
    mask = np.zeros(w.E, dtype=np.int32)
    mask[rng.choice(w.E, size=nreq, replace=False)] = 1
    k = w.k
    L = rng.uniform(-1, 1, (k, k))
    for coef in (E.COEF_PRIOR, E.COEF_PRIOR_RATE_EDGE, E.COEF_PRIOR_RATE):
        got = eng.frechet_matrices(L, coef)
        want = oracle.frechet(m, ow, L, 1.0, False, mask, precise=1).reshape(ow["C"], w.E, k, k).copy()
        for c in range(ow["C"]):
            for e in range(w.E):
                if coef == E.COEF_PRIOR_RATE_EDGE:
                    want[c, e] *= ow["cat_rates"][c] * m.edge_rates_csr[e]
                elif coef == E.COEF_PRIOR_RATE:
                    want[c, e] *= ow["cat_rates"][c]
        sel = mask.astype(bool)
        scale = np.max(np.abs(want[:, sel]), axis=(2, 3), keepdims=True)
        assert np.max(np.abs(got[:, sel] - want[:, sel]) / np.maximum(scale, 1e-300)) <= 1e-14


@pytest.mark.parametrize("cfg,S", [(3, 200_000), (2, 300_000), (5, 4096)])
def test_identities_at_scale(eng, cfg, S):
    """size-independent properties on a large batch:
       sum_s dwell(s) = 1 on every edge (sum_s F(e_s e_s^T) = F(I) = P), and
       d ll / d rate_e = E[transitions on e] - E[exit-rate dwell on e], both rate-weighted
       (Q = offdiag(Q) - diag(exit), F is linear in the direction, F(Q) = Q exp(Q))."""
    from phyly_amd import synth, engine as E
    w = synth.Workload(cfg)
    w.setup_engine(eng)
    codes = w.simulate(S)
    eng.set_patterns_codes(codes, w.defs)
    eng.set_site_weights(None)
    k = w.k
    ones, _ = eng.edge_expect(np.eye(k), E.COEF_PRIOR, want_sums=False)
    assert np.max(np.abs(ones - 1.0)) <= 1e-12
    Qn = w.prepare()["Qn"]
    tr, _ = eng.edge_expect(Qn * (1 - np.eye(k)), E.COEF_PRIOR_RATE, want_sums=False)
    dw, _ = eng.edge_expect(-np.diag(np.diag(Qn)), E.COEF_PRIOR_RATE, want_sums=False)
    d, _ = eng.deriv(want_sums=False)
    scale = np.maximum(np.max(np.abs(tr), axis=1, keepdims=True), np.max(np.abs(dw), axis=1, keepdims=True))
    assert np.max(np.abs((tr - dw) - d) / scale) <= 1e-11


# ------------------------------------------------------------------ JSON level, random models
def _run(kind, q):
    return json.loads(_prod(kind)(json.dumps(q)))


def _compare(kind, x, got, want):
    if kind == "em_update":
        # a ratio of two sums: where the denominator cancels to ~0 the ratio is ill conditioned; compare
        # rows whose oracle value is on the scale of the input rates
        rates = x["model_and_data"]["edge_rate_coefficients"]
        assert got["columns"] == want["columns"] and len(got["data"]) == len(want["data"])
        for a, b, r in zip(got["data"], want["data"], rates):
            assert a[0] == b[0]
            assert abs(a[1] - b[1]) <= 1e-10 * max(abs(b[1]), r) + 1e-300, (a, b)
    else:
        _check_table(got, want)


@pytest.mark.parametrize("kind,block", [(kind, b) for kind in cases.KINDS for b in range(cases.NBLOCKS)])
def test_random_inputs_match_oracle(oracle, kind, block):
    """60 seeded queries per command (expect_cases.feasible_query), every one of them compared:
    tests/test_expect_cases_cpu.py asserts that the oracle's values are all finite and what the 60 cover"""
    queries = cases.block(kind, block)
    assert len(queries) == cases.BLOCK
    for i, x in enumerate(queries):
        s = json.dumps(x)
        want = json.loads(_orc(oracle, kind)(s))
        assert all(np.isfinite(r[-1]) for r in want["data"]), i
        _compare(kind, x, json.loads(_prod(kind)(s)), want)


@pytest.mark.parametrize("name,kind,q", cases.INFEASIBLE, ids=[c[0] for c in cases.INFEASIBLE])
def test_zero_likelihood_is_refused(oracle, name, kind, q):
    """a selected site of likelihood zero (the reference never terminates there; the oracle prints a non-finite value):
    the product refuses, and afterwards the same engine answers the query without that site with the bits it gave before"""
    ok = json.dumps(cases.feasible_part(q))
    before = _prod(kind)(ok)
    _compare(kind, q, json.loads(before), json.loads(_orc(oracle, kind)(ok)))
    with pytest.raises(RuntimeError):
        _prod(kind)(json.dumps(q))
    assert _prod(kind)(ok) == before


@pytest.mark.parametrize("kind", cases.KINDS)
def test_duplicate_sites_expectations(oracle, kind):
    """the host layer evaluates each distinct site pattern once and maps sites to patterns (site_to_u) or weights the
    patterns (the sums path): 40 sites made of three patterns give the oracle's table under every site reduction, and
    without one, sites of the same pattern print the same bits"""
    order, queries = cases.duplicate_sites_queries(kind)
    for q in queries:
        got = _run(kind, q)
        _compare(kind, q, got, json.loads(_orc(oracle, kind)(json.dumps(q))))
        if "site_reduction" not in q:
            by_site = {}
            for row in got["data"]:
                by_site.setdefault(row[0], []).append(row[1:])
            assert sorted(by_site) == list(range(40))
            for s in range(40):
                assert by_site[s] == by_site[order.index(order[s])], s


# ------------------------------------------------------------------ known answers
def _vals(out):
    return np.array([r[-1] for r in out["data"]])


def _close(a, b, rel=1e-12):
    a, b = np.asarray(a, float), np.asarray(b, float)
    assert a.shape == b.shape
    assert np.all(np.abs(a - b) <= rel * np.abs(b)), (a, b)


def _exprel(x):
    x = np.asarray(x, float)
    safe = np.where(x == 0, 1.0, x)
    return np.where(x == 0, 1.0, np.expm1(safe) / safe)


BIRTH_SHARE = 1 / 2 - 1 / np.expm1(2.0)          # time share of state 1 on the edge of length 2 where 1 -> 2 happens
BIRTH_DWELL = {(0, 0): 0.5, (0, 1): 0.5, (0, 2): 0, (1, 0): 0, (1, 1): 1, (1, 2): 0,
               (2, 0): 0, (2, 1): BIRTH_SHARE, (2, 2): 1 - BIRTH_SHARE, (3, 0): 0, (3, 1): 0, (3, 2): 1}
BIRTH_EM = [1, 0, 1 / BIRTH_SHARE, 0]


def _check_known(got, want_rows, oracle_out):
    """rows [labels..., value]: 1e-12 relative where the known value is not 0; where it is 0 the product prints exactly
    0.0 if the oracle does (tests/test_expect_cases_cpu.py asserts that it does on every such row) and stays below 1e-14
    otherwise"""
    assert len(got["data"]) == len(want_rows) == len(oracle_out["data"])
    for a, w, o in zip(got["data"], want_rows, oracle_out["data"]):
        assert a[:-1] == list(w[:-1]) == o[:-1]
        if w[-1] != 0:
            assert abs(a[-1] - w[-1]) <= 1e-12 * abs(w[-1]), (a, w)
        elif o[-1] == 0.0:
            assert a[-1] == 0.0, (a, w)
        else:
            assert abs(a[-1]) <= 1e-14, (a, w)


def test_pure_birth_path_known_answers(oracle):
    """0 -> 1 -> 2 without return, states 0, 1, 1, 2, 2 observed along a path: one transition 0 -> 1 on edge 0 and one
    1 -> 2 on edge 2, nothing else; the time shares follow, and the EM update is transitions / exit-rate-weighted time"""
    d = cases.pure_birth_doc()
    s = json.dumps(d)
    want = [[0, e, a, b, 1.0 if (e, a, b) in ((0, 0, 1), (2, 1, 2)) else 0.0] for e in range(4) for a in range(3) for b in range(3) if a != b]
    _check_known(_run("trans", d), want, json.loads(oracle.arbplf_trans(s)))
    want = [[0, e, st, BIRTH_DWELL[(e, st)]] for e in range(4) for st in range(3)]
    _check_known(_run("dwell", d), want, json.loads(oracle.arbplf_dwell(s)))
    q = dict(d, site_reduction={"aggregation": "sum"})
    _check_known(_run("em_update", q), [[e, v] for e, v in enumerate(BIRTH_EM)], json.loads(oracle.arbplf_em_update(json.dumps(q))))


@pytest.mark.parametrize("kind", ["dwell", "em_update"])
def test_pure_birth_path_invariances(kind):
    """ten seeded relabellings of the nodes leave the table as it is; ten seeded permutations of the edge list permute
    the edge column with the rates and nothing else.  The product is not correctly rounded (a relabelled tree is walked
    in another order), so the tables are compared at 1e-12 relative, not bit for bit; a row that is 0 stays 0."""
    base = cases.pure_birth_doc()
    if kind == "em_update":
        base["site_reduction"] = {"aggregation": "sum"}
    ref = _run(kind, base)
    md = base["model_and_data"]
    rng = random.Random(20)
    for _ in range(10):
        lab = list(range(5))
        rng.shuffle(lab)
        y = copy.deepcopy(base)
        y["model_and_data"]["edges"] = [[lab[p], lab[c]] for p, c in md["edges"]]
        rows = [None] * 5
        for node in range(5):
            rows[lab[node]] = md["probability_array"][0][node]
        y["model_and_data"]["probability_array"] = [rows]
        got = _run(kind, y)
        assert [r[:-1] for r in got["data"]] == [r[:-1] for r in ref["data"]]
        _close(_vals(got), _vals(ref))
    ecol = ref["columns"].index("edge")
    for _ in range(10):
        perm = list(range(4))
        rng.shuffle(perm)
        y = copy.deepcopy(base)
        y["model_and_data"]["edges"] = [md["edges"][i] for i in perm]
        y["model_and_data"]["edge_rate_coefficients"] = [md["edge_rate_coefficients"][i] for i in perm]
        got = _run(kind, y)
        assert got["columns"] == ref["columns"] and len(got["data"]) == len(ref["data"])
        back = {tuple(r[:ecol] + [perm[r[ecol]]] + r[ecol + 1:-1]): r[-1] for r in got["data"]}     # new edge j is old edge perm[j]
        assert len(back) == len(ref["data"])
        _close([back[tuple(r[:-1])] for r in ref["data"]], _vals(ref))


@pytest.mark.parametrize("end_observed", [False, True], ids=["untruncated", "end_observed"])
def test_absorbing_path_known_answers(oracle, end_observed):
    """0 -> 1 without return along five edges (one of length 0), the root in state 0, cumulative lengths u, T = u[-1].
    Nothing observed below: the time to the transition is exponential, so edge (a, b) holds state 0 for the share
    exprel(b - a) exp(-b) and the transition with probability exp(-a) - exp(-b), and EM returns the rates it was given.
    Last node in state 1: the same conditioned on a transition before T.  The transition back never happens."""
    d = cases.absorbing_doc(end_observed)
    u = np.concatenate([[0.0], np.cumsum(cases.ABSORBING_RATES)])
    a, b, T = u[:-1], u[1:], u[-1]
    if end_observed:
        dwell_want = (_exprel(b - a) * np.exp(T - b) - 1) / np.expm1(T)

        def f(x):
            return (np.exp(-T) - np.exp(-x)) / np.expm1(-T)
        trans_want = f(a) - f(b)
    else:
        dwell_want = _exprel(b - a) * np.exp(-b)
        trans_want = np.exp(-a) - np.exp(-b)
    qd = dict(d, state_reduction={"selection": [0], "aggregation": "only"})
    dwell = _run("dwell", qd)
    assert dwell["columns"] == ["edge", "value"] and [r[0] for r in dwell["data"]] == list(range(5))
    _close(_vals(dwell), dwell_want)
    _check_table(dwell, json.loads(oracle.arbplf_dwell(json.dumps(qd))))
    trans = None
    for agg in ("sum", "avg", "only"):
        qt = dict(d, trans_reduction={"selection": [[0, 1]], "aggregation": agg})
        trans = _run("trans", qt)
        assert trans["columns"] == ["edge", "value"]
        assert _vals(trans)[3] == 0.0                       # the edge of length 0
        pos = trans_want != 0
        _close(_vals(trans)[pos], trans_want[pos])
        _check_table(trans, json.loads(oracle.arbplf_trans(json.dumps(qt))))
    back = _run("trans", dict(d, trans_reduction={"selection": [[1, 0]]}))
    assert back["columns"] == ["edge", "first_state", "second_state", "value"]
    assert [r[-1] for r in back["data"]] == [0.0] * 5
    em = _run("em_update", d)
    assert _vals(em)[3] == 0.0
    pos = np.array(cases.ABSORBING_RATES) > 0
    if end_observed:
        _close(_vals(em)[pos], (_vals(trans) / _vals(dwell))[pos])
    else:
        _close(_vals(em)[pos], np.array(cases.ABSORBING_RATES, float)[pos])
    _compare("em_update", d, em, json.loads(oracle.arbplf_em_update(json.dumps(d))))


def _both(oracle, kind, q):
    """the product's table, after it met the oracle's"""
    got = _run(kind, q)
    _check_table(got, json.loads(_orc(oracle, kind)(json.dumps(q))))
    return got


def test_trans_selection_and_aggregation_algebra(oracle):
    d = cases.algebra_doc()
    # `only` on one pair == `sum` on that pair, sites listed the other way round and matched by site
    only = _both(oracle, "trans", dict(d, trans_reduction={"selection": [[2, 1]], "aggregation": "only"}))
    rev = _both(oracle, "trans", dict(d, trans_reduction={"selection": [[2, 1]], "aggregation": "sum"}, site_reduction={"selection": [1, 0]}))
    assert only["columns"] == rev["columns"] == ["site", "edge", "value"]
    assert [r[0] for r in only["data"]] == [0] * 7 + [1] * 7 and [r[0] for r in rev["data"]] == [1] * 7 + [0] * 7
    _close([v for _, v in sorted((r[:2], r[2]) for r in rev["data"])], _vals(only))
    # all twelve pairs written out == the aggregation without a selection
    pairs = [[i, j] for i in range(4) for j in range(4) if i != j]
    for agg in ("sum", "avg"):
        listed = _both(oracle, "trans", dict(d, trans_reduction={"selection": pairs, "aggregation": agg}))
        implicit = _both(oracle, "trans", dict(d, trans_reduction={"aggregation": agg}))
        assert listed["columns"] == implicit["columns"] == ["site", "edge", "value"]
        _close(_vals(listed), _vals(implicit))
    one = _vals(_both(oracle, "trans", dict(d, trans_reduction={"aggregation": "sum"})))
    _close(_vals(_both(oracle, "trans", dict(d, trans_reduction={"aggregation": "avg"}))), one / 12)


MIX_RATES, MIX_PRIOR = [2, 3], [0.25, 0.75]
MIX_PAIRS, MIX_PAIR_WEIGHTS = [[0, 1], [3, 1], [2, 3]], [0.1, 4.2, 0.3]


@pytest.mark.parametrize("kind,third", [("trans", {"selection": MIX_PAIRS, "aggregation": MIX_PAIR_WEIGHTS}),
                                        ("trans", {"selection": MIX_PAIRS}),
                                        ("dwell", {"aggregation": [1.5, -0.5, 2, 1]})], ids=["trans-aggregated", "trans-listed", "dwell-weighted"])
def test_mixture_is_the_likelihood_weighted_combination(oracle, kind, third):
    """a two-category rate_mixture == the runs of its categories alone (edge rates scaled by the category rate), each
    site's rows weighted by prior x site likelihood of the category; the listed pairs are not in sorted order"""
    d = cases.algebra_doc()
    key = "trans_reduction" if kind == "trans" else "state_reduction"
    mixed = copy.deepcopy(d)
    mixed["model_and_data"]["rate_mixture"] = {"rates": MIX_RATES, "prior": MIX_PRIOR}
    got = _both(oracle, kind, dict(mixed, **{key: third}))
    if "aggregation" not in third:
        assert [r[2:4] for r in got["data"][:3]] == MIX_PAIRS
    parts, like = [], []
    for r in MIX_RATES:
        one = copy.deepcopy(d)
        one["model_and_data"]["edge_rate_coefficients"] = [r * v for v in d["model_and_data"]["edge_rate_coefficients"]]
        out = _both(oracle, kind, dict(one, **{key: third}))
        assert [row[:-1] for row in out["data"]] == [row[:-1] for row in got["data"]]
        parts.append(_vals(out))
        like.append(np.exp(_vals(json.loads(_prod("ll")(json.dumps(one))))))
    site = np.array([row[0] for row in got["data"]])
    w = [p * l[site] for p, l in zip(MIX_PRIOR, like)]
    _close(_vals(got), (w[0] * parts[0] + w[1] * parts[1]) / (w[0] + w[1]))


EM_MIXTURES = [{"rates": [0, 1.3], "prior": [0.3, 0.7]}, {"rates": [0.7, 0, 2.1], "prior": [0.2, 0.5, 0.3]},           # a rate-0 category
               {"rates": [0.5, 2], "prior": [1, 0]}, {"rates": [0.5, 2, 0], "prior": [0, 1, 0]},                       # all prior on one
               {"rates": [0, 2], "prior": [0, 1]},
               {"rates": [2.5], "prior": [1]}, {"rates": [0.4], "prior": "uniform_distribution"}]                       # one category, rate != 1


def _em_step_does_not_lose(q):
    ll0 = json.loads(_prod("ll")(json.dumps(q)))["data"][0][0]
    new = [r[1] for r in json.loads(_prod("em_update")(json.dumps(q)))["data"]]
    q2 = copy.deepcopy(q)
    q2["model_and_data"]["edge_rate_coefficients"] = new
    ll1 = json.loads(_prod("ll")(json.dumps(q2)))["data"][0][0]
    assert ll1 >= ll0 - 1e-12 * abs(ll0)
    return new


def test_em_update_increases_likelihood():
    """EM monotonicity on small random star trees (the property the reference checks in
    test_scripts/test_em_monotonicity.py), through the product's own ll and em-update; then on mixtures with a
    rate-0 category, with all the prior on one category, and with one category whose rate is not 1"""
    rng = np.random.default_rng(1234)
    for _ in range(8):
        n = int(rng.integers(2, 5))
        Q = float(rng.exponential()) * np.exp(rng.standard_normal((n, n)))
        np.fill_diagonal(Q, 0)
        S = int(rng.integers(1, 5))
        arr = np.exp(rng.standard_normal((S, 4, n)))
        md = {"edges": [[0, 1], [0, 2], [0, 3]], "edge_rate_coefficients": np.exp(rng.standard_normal(3)).tolist(),
              "rate_matrix": Q.tolist(), "probability_array": arr.tolist()}
        if rng.integers(2):
            c = int(rng.integers(1, 5))
            p = np.exp(rng.standard_normal(c))
            md["rate_mixture"] = {"rates": np.exp(rng.standard_normal(c)).tolist(), "prior": (p / p.sum()).tolist()}
        _em_step_does_not_lose({"model_and_data": md, "site_reduction": {"aggregation": "sum"}})
    rng = np.random.default_rng(4321)
    for mix in EM_MIXTURES:
        n = int(rng.integers(2, 5))
        Q = float(rng.exponential()) * np.exp(rng.standard_normal((n, n)))
        np.fill_diagonal(Q, 0)
        arr = np.exp(rng.standard_normal((3, 4, n)))
        md = {"edges": [[0, 1], [0, 2], [0, 3]], "edge_rate_coefficients": np.exp(rng.standard_normal(3)).tolist(),
              "rate_matrix": Q.tolist(), "probability_array": arr.tolist(), "rate_mixture": mix}
        new = _em_step_does_not_lose({"model_and_data": md, "site_reduction": {"aggregation": "sum"}})
        assert all(v > 0 for v in new)
