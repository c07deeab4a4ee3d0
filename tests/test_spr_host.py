"""CPU: plk_spr_moves (phyly_amd/csrc/host_spr.c) against the Python enumeration of tests/spr_cases.py.  Host only: no
engine and no GPU is touched."""
import numpy as np
import pytest

import spr_cases as cases
from helpers import K4_MODELS, k4_workload
from phyly_amd import engine as E_, synth


def _csr(edges):
    indptr, indices, _, _ = synth.csr_from_edges([list(map(int, e)) for e in edges])
    return np.asarray(indptr, dtype=np.int32), np.asarray(indices, dtype=np.int32)


def _small_trees():
    return {
        "star": [[0, i] for i in range(1, 7)],
        "two_leaves": [[0, 1], [0, 2]],
        "caterpillar": [[0, 1], [0, 2], [2, 3], [2, 4], [4, 5], [4, 6], [6, 7], [6, 8]],
        "unary_chain": [[0, 1], [1, 2], [2, 3], [3, 4]],
        "root_elsewhere": [[3, 0], [3, 4], [0, 1], [0, 2], [4, 5]],
    }


@pytest.mark.parametrize("name", list(K4_MODELS) + list(_small_trees()))
def test_moves_against_the_python_enumeration(name):
    edges = k4_workload(name).edges if name in K4_MODELS else _small_trees()[name]
    indptr, indices = _csr(edges)
    want = cases.moves_csr(indptr, indices)
    got = E_.spr_moves(indptr, indices)
    assert got.dtype == np.int32 and got.shape == (len(want), 2)
    assert [tuple(map(int, r)) for r in got] == want
    assert want == sorted(want) and len(set(want)) == len(want)          # ordered by p, then by e; nothing twice
    # the same moves in user indices, whichever way they are numbered
    assert sorted(cases.csr_to_user(edges, want)) == cases.moves_user(edges)
    lib = E_.load_library()
    assert lib.plk_spr_moves(len(indptr) - 1, E_._ptr(indptr), E_._ptr(indices), None) == len(want)      # the count-only call


def test_counts():
    wl = k4_workload("irregular")
    assert wl.N == 24 and len(cases.moves_user(wl.edges)) == 444
    assert len(E_.spr_moves(*_csr(wl.edges))) == 444
    t = _small_trees()
    assert len(E_.spr_moves(*_csr(t["two_leaves"]))) == 2                # each leaf onto the other's edge
    assert len(E_.spr_moves(*_csr(t["star"]))) == 6 * 5
    # a chain: the edge into node i can only go onto the i - 1 edges above it
    assert len(E_.spr_moves(*_csr(t["unary_chain"]))) == 0 + 1 + 2 + 3


def test_every_move_is_one_and_every_other_pair_is_none():
    edges = _small_trees()["caterpillar"]
    moves = set(cases.moves_user(edges))
    for p in range(-1, len(edges) + 1):
        for e in range(-1, len(edges) + 1):
            assert (cases.why_no_move(edges, p, e) is None) == ((p, e) in moves)
    assert "below" in cases.why_no_move(edges, 3, 5) and "pruned edge" in cases.why_no_move(edges, 3, 3)
    assert "range" in cases.why_no_move(edges, 0, 8)


def test_arrays_that_are_no_tree_give_no_moves():
    lib = E_.load_library()

    def count(indptr, indices):
        ip, ix = np.asarray(indptr, dtype=np.int32), np.asarray(indices, dtype=np.int32)
        out = np.full((64, 2), -7, dtype=np.int32)
        n = lib.plk_spr_moves(len(ip) - 1, E_._ptr(ip), E_._ptr(ix), E_._ptr(out))
        return n

    assert count([0, 2, 2, 2], [1, 2]) == 2                              # a tree, for comparison
    assert count([0], []) == 0                                           # no node
    assert count([0, 0], []) == 0                                        # one node, no edge
    assert count([1, 2, 2, 2], [1, 2]) == 0                              # indptr does not start at 0
    assert count([0, 2, 1, 2], [1, 2]) == 0                              # indptr decreases
    assert count([0, 1, 1, 1], [1]) == 0                                 # too few edges
    assert count([0, 2, 2, 2], [1, 1]) == 0                              # two edges into one node
    assert count([0, 2, 2, 2], [1, 3]) == 0                              # a child out of range
    assert count([0, 2, 2, 2], [0, 1]) == 0                              # an edge from a node to itself
    assert count([0, 1, 2, 3, 3], [3, 2, 1]) == 0                        # a cycle 1 -> 2 -> 1 beside the tree 0 -> 3
    assert lib.plk_spr_moves(3, None, None, None) == 0
