"""plk_nni_swaps (host only, no engine, no GPU) against the Python enumeration of tests/nni_cases.py."""
import numpy as np
import pytest

import nni_cases as cases
from helpers import K4_MODELS, k4_workload
from phyly_amd import engine as E_, synth


def _star(T):
    return [[T, i] for i in range(T)]


def _caterpillar(T):
    edges, top, nxt = [], 0, 1
    for _ in range(T - 1):
        edges += [[top, nxt], [top, nxt + 1]]
        top = nxt + 1
        nxt += 2
    return edges


TREES = {name: (lambda name=name: k4_workload(name).edges) for name in K4_MODELS}
TREES.update(star=lambda: _star(7), two_leaves=lambda: _star(2), caterpillar=lambda: _caterpillar(9),
             unary_chain=lambda: [[0, 1], [1, 2], [2, 3], [2, 4]])
COUNTS = dict(star=0, two_leaves=0, caterpillar=2 * 7, unary_chain=0)


@pytest.mark.parametrize("name", list(TREES))
def test_swaps_match_enumeration(name):
    edges = TREES[name]()
    indptr, indices, _, order = synth.csr_from_edges(edges)
    got = E_.nni_swaps(indptr, indices)
    want = cases.swaps_csr(indptr, indices)
    assert got.shape == (len(want), 2)
    assert [tuple(p) for p in got.tolist()] == want
    assert want == sorted(want) and len(set(want)) == len(want)
    if name in COUNTS:
        assert len(want) == COUNTS[name]
    else:
        assert len(want) > 0
    # the same set as the enumeration in the user's indices
    assert sorted(cases.csr_to_user(edges, want)) == cases.swaps_user(edges)
    # count only: no output buffer
    lib = E_.load_library()
    assert lib.plk_nni_swaps(len(indptr) - 1, E_._ptr(indptr), E_._ptr(indices), None) == len(want)


def test_no_tree_no_swaps():
    lib = E_.load_library()
    indptr = np.array([0, 2, 2], dtype=np.int32)             # two children claimed, three nodes missing
    indices = np.array([1, 1], dtype=np.int32)
    assert lib.plk_nni_swaps(2, E_._ptr(indptr), E_._ptr(indices), None) == 0
    assert lib.plk_nni_swaps(0, None, None, None) == 0
