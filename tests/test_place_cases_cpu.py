"""CPU: the references of tests/test_gpu_place.py can tell a right placement from a wrong one, and the host layer of
arbplf-place accepts and refuses what it should (arbplf_validate_string("place", ...): no GPU is touched).

Every case of the GPU file rewrites to a document the oracle parses, and an all-missing query reproduces the log
likelihood of the current tree on every edge.  Each plausible mistake of an implementation (place_cases.TEETH) moves some
site's reference value by more than MOVES = 1e-6 on every edge of the models it is run on, except the placements listed in
place_cases.STILL, which are asserted to move nothing and to be all of them."""
import ctypes
import json

import numpy as np
import pytest

import place_cases as cases
from helpers import K4_MODELS, QUERY_MODEL, family_workload, k4_workload, query_workload
from phyly_amd import engine as E_

SPLIT, PENDANT = 0.3, 0.07
_refs = {}


def _ref(oracle, key, build):
    if key not in _refs:
        md = build()
        _refs[key] = (md, cases.Reference(oracle, md))
    return _refs[key]


def _gpu_cases():
    """(key, builder) of every document tests/test_gpu_place.py places onto (at its smallest site count)"""
    out = [((name, 1), lambda name=name: cases.workload_doc(query_workload(name), 1, seed=1)) for name in list(K4_MODELS) + [QUERY_MODEL]]
    out += [(("family", k), lambda k=k: cases.workload_doc(family_workload(k), 3, seed=k)) for k in (2, 5, 13, 27, 48)]
    out += [(("ladder", k), lambda k=k: cases.ladder_doc(200, 2, seed=40 + k, k=k, C=2, leaf_scale=1e-4)) for k in (4, 13)]
    return out


@pytest.mark.parametrize("key,build", _gpu_cases(), ids=["-".join(map(str, key)) for key, _ in _gpu_cases()])
def test_document_builder(oracle, key, build):
    md, ref = _ref(oracle, key, build)
    data = np.asarray(md["character_data"])
    E, N = len(md["edges"]), len(md["edges"]) + 1
    miss = cases.missing_code(md)[1]
    cur = ref.current()
    worst = 0.0
    for e in range(E):
        md2 = cases.place_doc(md, e, [miss] * len(data), SPLIT, PENDANT)
        m2 = oracle.parse_model(md2)                            # a rooted tree again, two nodes and two edges more
        assert m2.N == N + 2 and m2.E == E + 2
        assert md2["edges"][e] == [md["edges"][e][0], N] and md2["edges"][E:] == [[N, md["edges"][e][1]], [N, N + 1]]
        r = md["edge_rate_coefficients"][e]
        assert md2["edge_rate_coefficients"][e] == SPLIT * r and md2["edge_rate_coefficients"][E:] == [(1.0 - SPLIT) * r, PENDANT]
        assert all(row[N] == miss and len(row) == N + 2 for row in md2["character_data"])
        # an all-missing query changes nothing: the two parts of the edge multiply to the whole
        got = ref.place(e, [miss] * len(data), SPLIT, PENDANT)
        err = float(np.max(np.abs(got - cur) / np.maximum(1.0, np.abs(cur))))
        worst = max(worst, err)
        assert err <= 1e-13, (key, e, err)
    print("%s: %d edges, all-missing query against the current tree: worst %.2e" % ("-".join(map(str, key)), E, worst))


def test_document_builder_appends_a_missing_definition_and_takes_dense_rows(oracle):
    import mixsens_cases
    md = mixsens_cases.five_taxon_doc(4, 4, seed=3)
    md["character_definitions"] = md["character_definitions"][:4]          # no all-ones row left
    md["character_data"] = [[c % 4 for c in row] for row in md["character_data"]]
    md2 = cases.place_doc(md, 2, [0, 1, 2, 3], 0.5, 0.1)
    assert md2["character_definitions"][4] == [1.0] * 4 and all(row[8] == 4 for row in md2["character_data"])
    assert oracle.parse_model(md2).N == 10
    dense = mixsens_cases.five_taxon_doc(4, 4, seed=3, dense=True)
    md3 = cases.place_doc(dense, 2, [[0.5, 0.25, 1.0, 0.0]] * 4, 0.5, 0.1)
    assert md3["probability_array"][0][8] == [1.0] * 4 and md3["probability_array"][0][9] == [0.5, 0.25, 1.0, 0.0]
    assert oracle.parse_model(md3).N == 10


# ---------------------------------------------------------------- teeth
S = 48


def _k4(oracle, name):
    return _ref(oracle, (name, S), lambda: cases.workload_doc(k4_workload(name), S, seed=7))


@pytest.mark.parametrize("tooth", cases.TEETH)
@pytest.mark.parametrize("name", ["irregular", "wide", "balanced32"])
def test_teeth(oracle, name, tooth):
    """the nonreversible_rates models with split = 0.3: A and B differ, and so do A^T G and (A B)^T G"""
    md, ref = _k4(oracle, name)
    q = cases.queries(md, np.asarray(md["character_data"]), 3)[0]
    still = cases.STILL.get((name, tooth), [])
    found = []
    for e in range(len(md["edges"])):
        d = cases.moved(ref.place(e, q, SPLIT, PENDANT, tooth), ref.place(e, q, SPLIT, PENDANT))
        if d <= cases.MOVES:
            found.append(e)
    assert found == still, (name, tooth, found)


def test_still_placements_are_what_the_table_says():
    """a rate-0 edge without data at either end (A = B = I, u and the new node share their state); an only child"""
    wl = k4_workload("irregular")
    e = wl.edges.index([20, 21])
    assert e == 16 and wl.edge_rates[e] == 0.0 and not {20, 21} & set(wl.data_nodes)
    assert wl.edges[12] == [15, 19] and sum(p == 15 for p, _ in wl.edges) == 1
    assert k4_workload("wide").edges == wl.edges
    b32 = [p for p, _ in k4_workload("balanced32").edges]
    assert all(b32.count(p) == 2 for p in b32)                  # no only child: the sibling tooth bites on every edge


def test_a_placement_moves_the_tree(oracle):
    """every placement of a query with data moves some site away from the current tree"""
    md, ref = _k4(oracle, "irregular")
    q = cases.queries(md, np.asarray(md["character_data"]), 3)[0]
    for e in range(len(md["edges"])):
        assert cases.moved(ref.place(e, q, SPLIT, PENDANT), ref.current()) > cases.MOVES


def test_edge_samples_hold_every_kind():
    for name in list(K4_MODELS) + [QUERY_MODEL]:
        md = cases.workload_doc(query_workload(name), 3, seed=1)
        kinds = cases.edge_kinds(md)
        have = set().union(*kinds.values())
        pick = cases.sample_edges(md, 16, seed=1)
        assert len(pick) == min(16, len(md["edges"])) and len(set(pick)) == len(pick)
        assert have <= set().union(*(kinds[e] for e in pick)), name
    irr = cases.edge_kinds(cases.workload_doc(query_workload("irregular"), 3, seed=1))
    assert set().union(*irr.values()) == {"root", "leaf", "data", "multi", "zero"}


# ---------------------------------------------------------------- host layer
@pytest.fixture(scope="module")
def validate():
    lib = E_.load_library()
    lib.arbplf_validate_string.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    lib.arbplf_validate_string.restype = ctypes.c_int
    return lambda doc: lib.arbplf_validate_string(b"place", json.dumps(doc).encode())


def _good():
    import mixsens_cases
    md = mixsens_cases.five_taxon_doc(6, 4, seed=5)
    pl = {"character_data": [[s % 6, 4] for s in range(6)], "edges": [3, 0, 6, 3], "split": 0.25, "pendant_rate": 0.1}
    dense = mixsens_cases.five_taxon_doc(6, 4, seed=5, dense=True)
    pd = {"probability_array": [[[0.5, 0.25, 1.0, 0.0], [1.0, 1.0, 1.0, 1.0]]] * 6, "pendant_rate": 0.0}
    return md, pl, dense, pd


def test_host_layer_accepts(validate, capfd):
    md, pl, dense, pd = _good()
    for doc in ({"model_and_data": md, "placement": pl},
                {"model_and_data": md, "placement": {k: v for k, v in pl.items() if k not in ("edges", "split")}},
                {"model_and_data": md, "placement": dict(pl, split=0), "site_reduction": {"aggregation": "sum"}},
                {"model_and_data": md, "placement": dict(pl, split=1.0), "site_reduction": {"selection": [4, 1]}},
                {"model_and_data": dense, "placement": pd},
                {"model_and_data": dense, "placement": dict(pd, edges=[6], split=0.9)}):
        assert validate(doc) == 0, capfd.readouterr().err
    capfd.readouterr()
    assert validate({"model_and_data": md, "placement": pl, "swaps": []}) != 0       # another command's key
    assert "swaps" in capfd.readouterr().err
    assert E_.load_library().arbplf_validate_string(b"nni", json.dumps({"model_and_data": md, "placement": pl}).encode()) != 0


def _bad_documents():
    md, pl, dense, pd = _good()

    def doc(**changes):
        p = dict(pl)
        for key, v in changes.items():
            if v is None:
                p.pop(key)
            else:
                p[key] = v
        return {"model_and_data": md, "placement": p}

    return [
        ("placement missing", {"model_and_data": md}, "placement"),
        ("placement no object", {"model_and_data": md, "placement": [1]}, "placement"),
        ("unknown key", doc(pendant=0.1), "pendant"),
        ("rows of unequal length", doc(character_data=[[0, 4]] * 5 + [[0]]), "unequal length"),
        ("row count", doc(character_data=[[0, 4]] * 5), "character_data"),
        ("character out of range", doc(character_data=[[0, 6]] * 6), "out of range"),
        ("negative character", doc(character_data=[[0, -1]] * 6), "out of range"),
        ("character not an integer", doc(character_data=[[0, 1.0]] * 6), "integer"),
        ("dense rows for a model with characters", {"model_and_data": md, "placement": dict(pd)}, "character_data"),
        ("characters for a dense model", {"model_and_data": dense, "placement": pl}, "probability_array"),
        ("both forms", doc(probability_array=pd["probability_array"]), "not both"),
        ("dense row too short", {"model_and_data": dense, "placement": dict(pd, probability_array=[[[0.5, 0.25, 1.0]]] * 6)}, "probability_array"),
        ("dense entry negative", {"model_and_data": dense, "placement": dict(pd, probability_array=[[[0.5, -0.25, 1.0, 0.0]]] * 6)}, "probability_array"),
        ("edge out of range", doc(edges=[3, 7]), "edges"),
        ("edge negative", doc(edges=[-1]), "edges"),
        ("edge not an integer", doc(edges=[3.0]), "edges"),
        ("edges no array", doc(edges=3), "edges"),
        ("split below 0", doc(split=-0.1), "split"),
        ("split above 1", doc(split=1.5), "split"),
        ("split a string", doc(split="half"), "split"),
        ("pendant_rate missing", doc(pendant_rate=None), "pendant_rate"),
        ("pendant_rate negative", doc(pendant_rate=-0.5), "pendant_rate"),
        # JSON has no spelling for a value that is not finite; the nearest a document gets is a literal that overflows,
        # which the JSON reader refuses before any key is looked at (its message names the line, not the key)
        ("pendant_rate not finite", doc(pendant_rate=1e999), "real number overflow"),
        ("pendant_rate a string", doc(pendant_rate="long"), "pendant_rate"),
        ("pendant_rate beyond the kernel's limit", doc(pendant_rate=1e300), "pendant_rate"),
    ]


BAD = _bad_documents()


def test_there_are_enough_bad_documents():
    assert len(BAD) >= 12


@pytest.mark.parametrize("what,doc,word", BAD, ids=[b[0].replace(" ", "_") for b in BAD])
def test_host_layer_refuses(validate, capfd, what, doc, word):
    capfd.readouterr()
    text = json.dumps(doc).replace("Infinity", "1e999")
    rc = E_.load_library().arbplf_validate_string(b"place", text.encode())
    err = capfd.readouterr().err
    assert rc != 0, what
    assert word in err, (what, err)
