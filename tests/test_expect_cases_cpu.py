"""CPU: the case lists of tests/test_gpu_expect.py are what tests/expect_cases.py says they are.  Every generated query
validates in the product's host layer and has only finite values in the oracle (so the GPU test compares every one of
them); the 60 cases of each command cover the paths a wrong driver could hide in; every INFEASIBLE document validates
and is non-finite in the oracle while the same document without its bad site is finite; the duplicate-site queries are
finite; and the oracle meets the closed forms, printing exactly 0.0 where the GPU test asserts == 0.0."""
import ctypes
import json
import math

import numpy as np
import pytest

import expect_cases as cases


def _orc(oracle, kind):
    return {"dwell": oracle.arbplf_dwell, "trans": oracle.arbplf_trans, "em_update": oracle.arbplf_em_update}[kind]


def _values(oracle, kind, q):
    return [r[-1] for r in json.loads(_orc(oracle, kind)(json.dumps(q)))["data"]]


@pytest.fixture(scope="module")
def validates():
    from phyly_amd import engine
    lib = engine.load_library()
    lib.arbplf_validate_string.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    return lambda kind, q: lib.arbplf_validate_string(kind.encode(), json.dumps(q).encode()) == 0


@pytest.mark.parametrize("kind", cases.KINDS)
def test_every_generated_query_is_feasible(oracle, validates, kind):
    got = cases.cases(kind)
    assert len(got) == cases.NCASES == cases.NBLOCKS * cases.BLOCK
    assert sum(len(cases.block(kind, b)) for b in range(cases.NBLOCKS)) == cases.NCASES
    for i, (x, _) in enumerate(got):
        assert validates(kind, x), i
        vals = _values(oracle, kind, x)
        assert vals and all(math.isfinite(v) for v in vals), i
        md = x["model_and_data"]
        assert len(md["edges"]) <= 12 and len(md["rate_matrix"]) <= 8
        assert len(md.get("character_data", md.get("probability_array"))) <= 8


def test_the_generator_is_deterministic():
    import random
    for kind in cases.KINDS:
        rng = random.Random(cases.SEEDS[kind])
        again = [cases.feasible_query(rng, kind)[0] for _ in range(3)]
        assert again == [x for x, _ in cases.cases(kind)[:3]]


@pytest.mark.parametrize("kind", cases.KINDS)
def test_coverage(kind):
    f = [facts for _, facts in cases.cases(kind)]

    def count(pred):
        return sum(1 for x in f if pred(x))
    assert count(lambda x: x["zero_rate_edge"]) >= 15
    assert count(lambda x: x["zero_in_Q"]) >= 15
    assert count(lambda x: x["zero_rate_category"]) >= 5
    for form in cases.FORMS:
        assert count(lambda x: form in x["forms"]) >= 15, form
    assert count(lambda x: x["k"] == 4) >= 15
    assert count(lambda x: x["k"] != 4) >= 15
    assert count(lambda x: x["k"] == 8) >= 3
    assert count(lambda x: x["edges"] >= 8) >= 10
    if kind == "trans":
        assert count(lambda x: x["many_listed_pairs_k4"]) >= 5
        assert count(lambda x: x["duplicate_pair"]) >= 5
        assert count(lambda x: x["aggregated_diagonal_pair"]) >= 5
    if kind == "dwell":
        assert count(lambda x: x["signed_state_weights"]) >= 5
        assert count(lambda x: x["state_avg"]) >= 5


def test_facts_are_read_off_the_query():
    """the coverage counts above rest on expect_cases.facts; pin it on documents written by hand"""
    md = {"edges": [[0, 1]], "edge_rate_coefficients": [0.0], "rate_matrix": [[0, 1, 0], [0, 0, 1], [1, 0, 0]],
          "rate_mixture": {"rates": [0, 2], "prior": [0.5, 0.5]}, "probability_array": [[[1, 1, 1], [1, 0, 0]]]}
    f = cases.facts({"model_and_data": md, "trans_reduction": {"selection": [[0, 1], [2, 2], [0, 1]], "aggregation": "sum"},
                     "state_reduction": {"aggregation": [1, -1, 0]}}, {"exact"})
    assert f["zero_rate_edge"] and f["zero_in_Q"] and f["zero_rate_category"] and f["duplicate_pair"]
    assert f["aggregated_diagonal_pair"] and f["signed_state_weights"] and not f["state_avg"] and not f["many_listed_pairs_k4"]
    md2 = dict(md, edge_rate_coefficients=[0.1], rate_matrix=[[0, 1, 1, 1], [1, 0, 1, 1], [1, 1, 0, 1], [1, 1, 1, 0]])
    del md2["rate_mixture"]
    f = cases.facts({"model_and_data": md2, "trans_reduction": {"selection": [[0, 1], [1, 2], [2, 3], [3, 0], [2, 2]]},
                     "state_reduction": {"aggregation": "avg"}}, set())
    assert not (f["zero_rate_edge"] or f["zero_in_Q"] or f["zero_rate_category"] or f["duplicate_pair"] or f["aggregated_diagonal_pair"])
    assert f["many_listed_pairs_k4"] and f["state_avg"] and f["k"] == 4 and f["edges"] == 1
    md2["gamma_rate_mixture"] = {"gamma_shape": 1.0, "gamma_categories": 2, "invariable_prior": 0.2}
    assert cases.facts({"model_and_data": md2}, set())["zero_rate_category"]


@pytest.mark.parametrize("name,kind,q", cases.INFEASIBLE, ids=[c[0] for c in cases.INFEASIBLE])
def test_infeasible_documents(oracle, validates, name, kind, q):
    assert validates(kind, q)
    assert any(not math.isfinite(v) for v in _values(oracle, kind, q))
    ok = cases.feasible_part(q)
    assert validates(kind, ok)
    vals = _values(oracle, kind, ok)
    assert vals and all(math.isfinite(v) for v in vals)


def test_infeasible_list():
    assert len(cases.INFEASIBLE) >= 6
    for cause in ("zero_rate_edge", "zero_rate_category", "forbidden_transition", "zero_root_row"):
        for tag in ("alone", "among"):
            assert any(n.startswith(cause + "-" + tag) for n, _, _ in cases.INFEASIBLE)
    assert {kind for _, kind, _ in cases.INFEASIBLE} == set(cases.KINDS)


@pytest.mark.parametrize("kind", cases.KINDS)
def test_duplicate_site_queries_are_feasible(oracle, kind):
    order, queries = cases.duplicate_sites_queries(kind)
    assert len(order) == 40 and len(queries) == (2 if kind == "em_update" else 4)
    for q in queries:
        md = q["model_and_data"]
        sites = md[cases.DUPLICATE_FORM[kind]]
        assert len(sites) == 40 and len({repr(s) for s in sites}) == 3
        assert all(math.isfinite(v) for v in _values(oracle, kind, q))


# ------------------------------------------------------------------ closed forms, oracle side
def exprel(x):
    x = np.asarray(x, float)
    safe = np.where(x == 0, 1.0, x)
    return np.where(x == 0, 1.0, np.expm1(safe) / safe)


def test_pure_birth_path_oracle(oracle):
    """the rows the GPU test compares with == 0.0 are printed as exactly 0.0 by the oracle"""
    d = cases.pure_birth_doc()
    tr = json.loads(oracle.arbplf_trans(json.dumps(d)))
    assert tr["columns"] == ["site", "edge", "first_state", "second_state", "value"] and len(tr["data"]) == 24
    for site, edge, a, b, v in tr["data"]:
        if (edge, a, b) in ((0, 0, 1), (2, 1, 2)):
            assert v == pytest.approx(1.0, rel=1e-15)
        else:
            assert v == 0.0, (edge, a, b)
    dw = {(r[1], r[2]): r[3] for r in json.loads(oracle.arbplf_dwell(json.dumps(d)))["data"]}
    share = 1 / 2 - 1 / math.expm1(2)
    assert share == pytest.approx(0.343482357250334, rel=1e-14)
    want = {(0, 0): 0.5, (0, 1): 0.5, (0, 2): 0, (1, 0): 0, (1, 1): 1, (1, 2): 0, (2, 0): 0, (2, 1): share, (2, 2): 1 - share,
            (3, 0): 0, (3, 1): 0, (3, 2): 1}
    for key, w in want.items():
        if w == 0:
            assert dw[key] == 0.0, key
        else:
            assert dw[key] == pytest.approx(w, rel=1e-14), key
    em = _values(oracle, "em_update", dict(d, site_reduction={"aggregation": "sum"}))
    assert em[1] == 0.0 and em[3] == 0.0
    assert [em[0], em[2]] == pytest.approx([1, 1 / share], rel=1e-14)


@pytest.mark.parametrize("end_observed", [False, True])
def test_absorbing_path_oracle(oracle, end_observed):
    d = cases.absorbing_doc(end_observed)
    u = np.concatenate([[0.0], np.cumsum(cases.ABSORBING_RATES)])
    a, b, T = u[:-1], u[1:], u[-1]
    dwell0 = np.array(_values(oracle, "dwell", dict(d, state_reduction={"selection": [0], "aggregation": "only"})))
    if end_observed:
        want = (exprel(b - a) * np.exp(T - b) - 1) / math.expm1(T)
    else:
        want = exprel(b - a) * np.exp(-b)
    np.testing.assert_allclose(dwell0, want, rtol=1e-14)
    back = _values(oracle, "trans", dict(d, trans_reduction={"selection": [[1, 0]]}))
    assert back == [0.0] * 5
    em = _values(oracle, "em_update", d)
    assert em[3] == 0.0
    if not end_observed:
        np.testing.assert_allclose(em, cases.ABSORBING_RATES, rtol=1e-14)
