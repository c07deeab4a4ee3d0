"""CPU: the folded op stream of the streamed-code k = 4 interpreter (plk_v4s_fold_ops, plk_fused_v4s_fold and the replay
check plk_fused_check_v4s_fold in phyly_amd/csrc/plk_program.h) under AddressSanitizer + UBSan.

tests/foldcheck_main.cpp is a stand-alone program: over the seeded random trees of tests/progcheck_main.cpp it folds the
checked stream, requires the replay check to accept the fold and to refuse four kinds of corrupted folds, unfolds it back
to the checked stream's words, and looks at what keeps a dispatch of its own.  On the tree of BASELINE config 3 (written
here from synth.Workload(3)) it also pins the dispatch counts of one category: 161 before the fold.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "phyly_amd", "csrc")


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fold") / "foldcheck")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-I", CSRC, "-o", out, os.path.join(ROOT, "tests", "foldcheck_main.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


def test_fold_random_trees_and_config3(binary, tmp_path):
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
    tag, before, after = lines[0].split()
    # 161 dispatches a category before the fold; 16 ADVANCEs and at least 8 of the 10 SCALEs folded, and the shorter stream
    # has fewer REFILLs
    assert tag == "config3" and int(before) == 161 and int(after) <= 161 - 16 - 8
    out = lines[1].split()
    assert out[0] == "ok"
    trees, adv, scale, left, c_kind, c_scale, c_drop, c_refill = (int(v) for v in out[1:])
    # about half of the generator's trees fit the 4-slot stack and the LDS; both folds and a SCALE that keeps its own
    # dispatch occur, and every negative control ran on many trees
    assert trees >= 1500 and adv > 1000 and scale > 0 and left > 0
    assert c_kind > 500 and c_scale > 100 and c_drop == trees and c_refill == trees
