"""CPU: the four-leaf tables of the streamed k = 4 interpreter (plk_v4q_candidates, plk_fused_v4q_build, the replay check
plk_fused_check_v4q, the rank tables and the plan plk_v4q_plan in phyly_amd/csrc/plk_program.h) under AddressSanitizer + UBSan.

tests/quadcheck_main.cpp is a stand-alone program: over the two five-leaf shapes, the four-leaf trees whose node is the root,
the four followers of the absorbed product, a third child, data inside the run, a leaf with five occurring codes, a 40-leaf
caterpillar and 120 random trees, with nchar 4, 5 and 16 and occurring codes that are contiguous, scattered ({1, 5, 9, 15}),
different from leaf to leaf, single, or without code 0, it derives the rewritten formats, requires every replay check to
accept them, the root never to be absorbed, the SCALE ops to stay, the matrix stream to shrink by the absorbed products, padded
sites to land on rank 0, and a host interpreter of the handlers' fp64 sequences to give the same bits as on the checked
program; seven deliberately wrong formats or row builders must each fail (the rows in double-double among them), and a
SCALE put by hand into the run of either shape leaves no candidate, an untouched program and a refused forced table.  On the tree of BASELINE config 3 (written here
from synth.Workload(3), whose leaves take codes 0 .. 3 of 5) the plan at 10M sites is set against the unit budget.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "phyly_amd", "csrc")


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("quad") / "quadcheck")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-I", CSRC, "-o", out, os.path.join(ROOT, "tests", "quadcheck_main.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


def test_quad_shapes_and_config3(binary, tmp_path):
    from phyly_amd import synth
    wl = synth.Workload(3)
    assert wl.nchar == 5
    # the simulated alignment takes codes 0 .. 3 at every leaf: what the plan below is handed as occurring codes
    codes = wl.simulate(2000)
    leaf = wl.indptr[1:] == wl.indptr[:-1]
    assert all(set(codes[a].tolist()) <= {0, 1, 2, 3} for a in range(wl.N) if leaf[a])
    tree = tmp_path / "config3.tree"
    with open(tree, "w") as f:
        f.write("%d\n" % wl.N)
        for arr in (wl.indptr, wl.indices, wl.preorder):
            f.write(" ".join(str(int(v)) for v in arr) + "\n")
    r = subprocess.run([binary, str(tree)], capture_output=True, text=True, env=ENV, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.split("\n")
    tag, *nums = lines[0].split()
    nA, nB, groups, quads, triples, units, mats, nobs, small, only3, never = (int(v) for v in nums)
    assert tag == "config3"
    # the shapes counted from the tree itself: non-root nodes with two children and four leaves below them
    kids = [list(wl.indices[wl.indptr[a]:wl.indptr[a + 1]]) for a in range(wl.N)]
    cherry = [len(k) == 2 and not kids[k[0]] and not kids[k[1]] for k in kids]
    three = [len(k) == 2 and any(cherry[k[i]] and not kids[k[1 - i]] for i in (0, 1)) for k in kids]
    root = wl.preorder[0]
    A = [a for a in range(wl.N) if a != root and len(kids[a]) == 2 and any(three[kids[a][i]] and not kids[kids[a][1 - i]] for i in (0, 1))]
    B = [a for a in range(wl.N) if a != root and len(kids[a]) == 2 and cherry[kids[a][0]] and cherry[kids[a][1]]]
    assert (nA, nB) == (len(A), len(B)) == (10, 4)
    # a group per category, every four-leaf node and the 6 three-leaf nodes that are not below one:
    # 200 units + 10 x (52 - 7) + 4 x (52 - 10) + 6 x 19 = 932 units of 160 B, with 4608 B of static LDS within 156 KB
    assert (groups, quads, triples) == (4, 14, 6)
    assert units == 200 + 10 * 45 + 4 * 42 + 6 * 19 == 932 and units * 160 + 4608 <= 156 * 1024
    # 65 products and 67 look-ups in the pair-table program: a shape-A table stands for two products and three look-ups, a
    # shape-B table for one product and two look-ups, a three-leaf table for one product and two look-ups
    assert mats == 65 - (2 * 10 + 4 + 6) and nobs == 67 - (2 * 10 + 4 + 6) == 37
    # not at 300 sites by default, not under + 1024 alone (three-leaf tables only), not under + 32768
    assert (small, only3, never) == (0, 0, 0)
    out = lines[1].split()
    assert out[0] == "ok"
    cases, tA, tB, tri, c_swap, c_lut, c_matrix, c_short, c_dd, c_edges, c_order, c_scale = (int(v) for v in out[1:])
    assert cases > 250 and tA > 100 and tB > 40 and tri > 30
    # double-double rows: required to differ wherever every leaf takes two codes or more (inside the program), counted elsewhere
    assert min(c_swap, c_lut, c_matrix, c_short, c_dd, c_edges) > 100 and c_order > 60
    # a SCALE inside the run: before MATVEC(e_t) and before MATVEC(e_d) of shape A, between POPMUL and MATVEC of shape B, at nchar 4, 5, 16
    assert c_scale == 3 * 3
