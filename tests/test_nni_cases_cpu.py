"""CPU: the references of tests/test_gpu_nni.py can tell a right swap from a wrong one.  Every listed pair rewrites to a
tree the oracle parses; pairs that are no swap are refused; on `irregular` and `balanced32` each plausible mistake of an
implementation moves some site's reference ll by more than 1e-6, and so does every swap itself.

Swaps that move nothing: nni_cases.STILL_SWAPS, two swaps across the rate-0 edge of the irregular tree (`irregular` and
`wide`); every other swap of those models and of `balanced32` moves some site by more than 1e-6 from the current tree
(test_every_swap_moves)."""
import numpy as np
import pytest

import nni_cases as cases
from helpers import K4_MODELS, k4_workload

TEETH_MODELS = ("irregular", "balanced32")
MOVE_MODELS = TEETH_MODELS + ("wide",)        # every model that has an entry in nni_cases.STILL_SWAPS is checked here
S = 48
_refs = {}


def _ref(oracle, name):
    if name not in _refs:
        wl = k4_workload(name)
        md = cases.workload_doc(wl, S, seed=7)
        _refs[name] = (cases.Reference(oracle, md), cases.swaps_user(md["edges"]))
    return _refs[name]


@pytest.mark.parametrize("name", K4_MODELS)
def test_every_pair_rewrites_to_a_tree(oracle, name):
    wl = k4_workload(name)
    md = cases.workload_doc(wl, 2)
    sw = cases.swaps_user(md["edges"])
    assert sw
    deg = np.bincount([p for p, _ in md["edges"]], minlength=wl.N)
    for a, b in sw:
        md2 = cases.swap_doc(md, a, b)
        m2 = oracle.parse_model(md2)                      # a rooted tree again
        assert m2.N == wl.N and m2.E == wl.E
        assert np.array_equal(np.bincount([p for p, _ in md2["edges"]], minlength=wl.N), deg)     # every node keeps its degree
        assert [e[1] for e in md2["edges"]] == [e[1] for e in md["edges"]]
        assert sum(x != y for x, y in zip(md2["edges"], md["edges"])) == 2


def test_pairs_that_are_no_swap():
    edges = k4_workload("irregular").edges
    into = cases.in_edges(edges)
    a, b = cases.swaps_user(edges)[5]
    v = edges[a][0]
    deep = next(e for e, (p, c) in enumerate(edges) if p in into and into[p][1] in into and into[into[p][1]][1] == edges[b][0])
    for pair, word in (((a, a), "twice"), ((a, into[v][0]), "ends where"), ((deep, b), "child"), ((b, a), ""),
                       ((a, len(edges)), "range"), ((-1, b), "range"), ((1.0, b), "integers")):
        assert cases.why_no_swap(edges, *pair) is not None, pair
        assert word in cases.why_no_swap(edges, *pair)
        with pytest.raises(ValueError):
            cases.swap_edges(edges, *pair)


def test_moved_matrices_are_the_rewritten_documents(oracle):
    """Reference moves the transition matrices of the original to the CSR positions of the rewritten document; the oracle's
    own preparation of that document gives the same numbers"""
    ref, sw = _ref(oracle, "irregular")
    for a, b in sw[::7]:
        md2 = cases.swap_doc(ref.md, a, b)
        m2, w2 = ref.model(md2)
        w_own = oracle.prepare(oracle.parse_model(md2))
        assert np.array_equal(w2["P"], w_own["P"])
        assert np.array_equal(ref.swap(a, b), oracle.site_ll(m2, w_own, B=m2.B, precise=1)[0])


@pytest.mark.parametrize("name", MOVE_MODELS)
def test_every_swap_moves(oracle, name):
    ref, sw = _ref(oracle, name)
    cur = ref.current()
    still = [p for p in sw if cases.moved(ref.swap(*p), cur) <= cases.MOVES]
    assert still == cases.STILL_SWAPS.get(name, []), still
    assert len(still) <= len(sw) // 10
    assert set(cases.STILL_SWAPS) <= set(MOVE_MODELS)


@pytest.mark.parametrize("name", TEETH_MODELS)
def test_teeth(oracle, name):
    ref, sw = _ref(oracle, name)
    edges = ref.md["edges"]
    data_nodes = set(getattr(k4_workload(name), "data_nodes", ()))
    C = ref.w["P"].shape[0]
    bitten = dict(rates=0, data=0, sibling=0, categories=0)
    for a, b in sw:
        right = ref.swap(a, b)
        ra, rb = ref.md["edge_rate_coefficients"][a], ref.md["edge_rate_coefficients"][b]
        if abs(ra - rb) > 0.02:
            assert cases.moved(ref.wrong_rates_stay(a, b), right) > cases.MOVES, (a, b)
            bitten["rates"] += 1
        if edges[a][0] in data_nodes:
            assert cases.moved(ref.wrong_data_dropped(a, b), right) > cases.MOVES, (a, b)
            bitten["data"] += 1
        wrong, below = ref.wrong_sibling_left_out(a, b)
        if below:
            assert cases.moved(wrong, right) > cases.MOVES, (a, b)
            bitten["sibling"] += 1
        if C > 1 and ra > 0:
            assert cases.moved(ref.wrong_categories_exchanged(a, b), right) > cases.MOVES, (a, b)
            bitten["categories"] += 1
    # each tooth bites where the model has what it needs: data on internal nodes and several categories on `irregular` only
    assert bitten["rates"] > len(sw) // 2 and bitten["sibling"] > len(sw) // 2
    assert (bitten["data"] > 0) == bool(data_nodes)
    assert (bitten["categories"] > 0) == (C > 1)
