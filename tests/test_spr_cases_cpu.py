"""CPU: the references of tests/test_gpu_spr.py can tell a right prune-and-regraft move from a wrong one.

Two identities of the move hold in the oracle: (I1) a move with split = 0 onto a sibling edge of p gives the log
likelihood of the current tree; (I2) a move whose x is a leaf equals the placement of that leaf's column onto the target in
the tree without the leaf and p, w kept, with pendant_rate = r_p.  Each plausible mistake of an implementation
(spr_cases.TEETH) moves some site's reference value by more than MOVES = 1e-6 on every sampled move it has something to say
about, except the moves listed in STILL, which are asserted to be all of them."""
import numpy as np
import pytest

import place_cases
import spr_cases as cases
from helpers import K4_MODELS, QUERY_MODEL, k4_workload, query_workload

SPLIT = 0.3
S = 48
_refs = {}


def _k4(oracle, name, sites=S):
    if (name, sites) not in _refs:
        md = cases.workload_doc(k4_workload(name), sites, seed=7)
        _refs[name, sites] = (md, cases.Reference(oracle, md))
    return _refs[name, sites]


# ---------------------------------------------------------------- the document builder
@pytest.mark.parametrize("name", list(K4_MODELS) + [QUERY_MODEL])
def test_document_builder(oracle, name):
    md = cases.workload_doc(query_workload(name), 2, seed=1)
    E, N = len(md["edges"]), len(md["edges"]) + 1
    miss = cases.missing_code(md)[1]
    for p, e in cases.sample_moves(md, 48, seed=1):
        md2 = cases.move_doc(md, p, e, SPLIT)
        m2 = oracle.parse_model(md2)                            # a rooted tree again, one node and one edge more
        assert m2.N == N + 1 and m2.E == E + 1
        (u, b), x = md["edges"][e], md["edges"][p][1]
        assert md2["edges"][e] == [u, N] and md2["edges"][p] == [N, x] and md2["edges"][E:] == [[N, b]]
        r = md["edge_rate_coefficients"][e]
        assert md2["edge_rate_coefficients"][e] == SPLIT * r and md2["edge_rate_coefficients"][E:] == [(1.0 - SPLIT) * r]
        assert md2["edge_rate_coefficients"][p] == md["edge_rate_coefficients"][p]
        assert all(row[N] == miss and len(row) == N + 1 for row in md2["character_data"])
    with pytest.raises(ValueError):
        cases.move_doc(md, 0, 0, SPLIT)


def test_samples_hold_every_kind():
    for name in list(K4_MODELS) + [QUERY_MODEL]:
        md = cases.workload_doc(query_workload(name), 3, seed=1)
        pick = cases.sample_moves(md, 48, seed=1)
        assert len(pick) == 48 and len(set(pick)) == 48
        assert cases.tree_kinds(md) <= cases.tree_kinds(md, pick), name
    irr = cases.workload_doc(query_workload("irregular"), 3, seed=1)
    assert cases.tree_kinds(irr) == set(cases.KINDS)
    assert len(cases.moves_user(irr["edges"])) == 444


# ---------------------------------------------------------------- the identities
@pytest.mark.parametrize("name", ["irregular", "wide", "balanced32"])
def test_split_0_onto_a_sibling_is_the_current_tree(oracle, name):
    """(I1)"""
    md, ref = _k4(oracle, name, 5)
    cur = ref.current()
    n, worst = 0, 0.0
    for p, e in cases.moves_user(md["edges"]):
        if md["edges"][p][0] != md["edges"][e][0]:
            continue
        got = ref.move(p, e, 0.0)
        err = float(np.max(np.abs(got - cur) / np.maximum(1.0, np.abs(cur))))
        worst = max(worst, err)
        n += 1
        assert err <= 1e-13, (name, p, e, err)
    parents = [int(a) for a, _ in md["edges"]]
    assert n == sum(parents.count(a) - 1 for a in parents) > 0      # every edge with every sibling
    print("%s: %d sibling moves at split 0 against the current tree: worst %.2e" % (name, n, worst))


def _without_leaf(md, p):
    """the document without the leaf x below user edge p and without p; (document, user edge -> its index there)"""
    x = int(md["edges"][p][1])
    sh = lambda y: y - (y > x)                                  # noqa: E731
    edges = [[sh(int(a)), sh(int(b))] for i, (a, b) in enumerate(md["edges"]) if i != p]
    out = dict(md, edges=edges, edge_rate_coefficients=[r for i, r in enumerate(md["edge_rate_coefficients"]) if i != p])
    out["character_data"] = [[c for y, c in enumerate(row) if y != x] for row in md["character_data"]]
    return out, {e: e - (e > p) for e in range(len(md["edges"])) if e != p}


def test_a_leaf_move_is_a_placement(oracle):
    """(I2) on every leaf x of `irregular`, four targets each"""
    md, ref = _k4(oracle, "irregular", 5)
    t = cases.Tree(md["edges"])
    rng = np.random.default_rng(2)
    worst, n = 0.0, 0
    for p, (w, x) in enumerate(t.edges):
        if x in t.kids:
            continue
        small, at = _without_leaf(md, p)
        pref = place_cases.Reference(oracle, small)
        targets = [e for q, e in cases.moves_user(md["edges"]) if q == p]
        column = [row[x] for row in md["character_data"]]
        for e in rng.choice(targets, 4, replace=False):
            want = pref.place(at[int(e)], column, SPLIT, float(md["edge_rate_coefficients"][p]))
            got = ref.move(p, int(e), SPLIT)
            err = cases.site_err(got, want)
            worst = max(worst, err)
            n += 1
            assert err <= 1e-13, (p, int(e), err)
    assert n >= 4 * 10
    print("irregular: %d leaf moves against placements: worst %.2e" % (n, worst))


# ---------------------------------------------------------------- teeth
# Sampled moves (user indices) on which a tooth that has something to say cannot bite, asserted to be all of them.
# The irregular tree (K4_MODELS irregular and wide): the edge 20 -> 21 (user index 16) has rate 0, so both of its parts
# are the identity whatever the split, and under such an edge without data at either end the subtree hangs from u as well
# as from the new node.
STILL = {
    ("irregular", "ab_exchanged"): [(8, 16), (9, 16)], ("wide", "ab_exchanged"): [(8, 16), (9, 16)],
    ("irregular", "attached_at_u"): [(8, 16), (9, 16)], ("wide", "attached_at_u"): [(8, 16), (9, 16)],
}


@pytest.mark.parametrize("tooth", cases.TEETH)
@pytest.mark.parametrize("name", ["irregular", "wide", "balanced32"])
def test_teeth(oracle, name, tooth):
    md, ref = _k4(oracle, name)
    found, said = [], 0
    for p, e in cases.sample_moves(md, 48, seed=3):
        wrong = ref.move(p, e, SPLIT, tooth)
        if wrong is None:
            continue
        said += 1
        if cases.moved(wrong, ref.move(p, e, SPLIT)) <= cases.MOVES:
            found.append((p, e))
    assert said >= 4, (name, tooth, said)                       # the tooth has something to say about some of them
    assert found == STILL.get((name, tooth), []), (name, tooth, found)
