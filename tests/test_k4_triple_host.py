"""CPU: the three-leaf tables of the streamed k = 4 interpreter (plk_fused_v4t_build, the replay check plk_fused_check_v4t,
the row function plk_v4t_row and the plan plk_v4t_plan in phyly_amd/csrc/plk_program.h) under AddressSanitizer + UBSan.

tests/triplecheck_main.cpp is a stand-alone program: over caterpillars and balanced trees of 3 .. 12 leaves and a 40-leaf
caterpillar, the children of every node in both orders, nchar 4, 5, 6 (and 7, 16, where the form must not apply), C 1 .. 4 in
1, 2 and C groups and LDS bounds from nothing to everything, it derives the rewritten formats, requires every replay check to
accept them, the root never to be absorbed, the SCALE ops to stay where they were, the matrix stream to shrink by exactly
the absorbed nodes, and a host interpreter of the handlers' fp64 sequences to give the same bits as on the checked program;
six deliberately wrong builders must each fail.  On the tree of BASELINE config 3 (written here from synth.Workload(3)) the
nodes the plan absorbs are set against the byte budget.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "phyly_amd", "csrc")


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("triple") / "triplecheck")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-I", CSRC, "-o", out, os.path.join(ROOT, "tests", "triplecheck_main.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


def test_triple_shaped_trees_and_config3(binary, tmp_path):
    from phyly_amd import synth
    wl = synth.Workload(3)
    assert wl.nchar == 5
    tree = tmp_path / "config3.tree"
    with open(tree, "w") as f:
        f.write("%d\n" % wl.N)
        for arr in (wl.indptr, wl.indices, wl.preorder):
            f.write(" ".join(str(int(v)) for v in arr) + "\n")
    r = subprocess.run([binary, str(tree)], capture_output=True, text=True, env=ENV, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.split("\n")
    tag, cand, units, mats, g1, g2, gc, mats_g2, dflt_groups, dflt_nodes, small_nodes = lines[0].split()
    cand, units, mats, g1, g2, gc, mats_g2 = (int(v) for v in (cand, units, mats, g1, g2, gc, mats_g2))
    assert tag == "config3"
    # nodes whose children are a cherry and a leaf, counted from the tree itself: none of them is the root
    kids = [list(wl.indices[wl.indptr[a]:wl.indptr[a + 1]]) for a in range(wl.N)]
    cherry = [len(k) == 2 and not kids[k[0]] and not kids[k[1]] for k in kids]
    leaf = [not k for k in kids]
    nodes = [a for a in range(wl.N) if len(kids[a]) == 2 and any(cherry[kids[a][i]] and leaf[kids[a][1 - i]] for i in (0, 1))]
    assert wl.preorder[0] not in nodes and cand == len(nodes) == 16
    # the byte budget: 156 KB of LDS over the resident categories, less one category's image, in tables of
    # (nchar^2 - nchar - 1) units of nchar * 32 bytes more than the cherry and the leaf they replace
    per, image, limit = (25 - 5 - 1) * 160, units * 160, 156 * 1024
    want = lambda resident: min(cand, (limit // resident - image) // per)
    assert (g1, g2, gc) == (want(4), want(2), want(1)) == (2, 15, 16)
    assert mats == 65 and mats_g2 == mats - g2
    # the default: at the benchmark's 10M sites two groups, the fastest of the three forced forms (profiles/ll_k4_triple_ab.json);
    # at 300 sites not the form
    assert int(small_nodes) == 0
    assert (int(dflt_groups), int(dflt_nodes)) == (2, g2)
    out = lines[1].split()
    assert out[0] == "ok"
    cases, tables, none, c_radix, c_matrix, c_scale, c_root, c_swap, c_edge = (int(v) for v in out[1:])
    # 42 trees x 5 nchar x 6 bounds and config 3; every control ran on many trees (a SCALE needs a long caterpillar or the
    # config 3 tree; the root control a tree whose root joins a cherry and a leaf)
    assert cases > 700 and tables > 400 and none > 300
    assert min(c_radix, c_matrix, c_swap) > 90 and c_edge > 50 and c_scale >= 3 and c_root >= 6
