"""CPU: the pair-product op stream of the streamed k = 4 interpreter (k_ll_fused4_v4s<768, true, true>; plk_fused_v4p_build and the replay
check plk_fused_check_v4p in phyly_amd/csrc/plk_program.h) under AddressSanitizer + UBSan.

tests/pairmulcheck_main.cpp is a stand-alone program: over the seeded random trees of tests/progcheck_main.cpp (nchar 4, 5
and 16) it derives the stream from the checked one, requires the replay check to accept it and to refuse seven kinds of
corrupted streams (a flipped parity and a wrong table field for exactly that reason), walks it next to the checked stream on its own, compares the handler numbering of
plk_program.h with the generated header's, and requires every observation and PAIR handler of the
table to occur.  Programs that need 4 stack slots must get no such stream.  On the tree of BASELINE config 3 (written here
from synth.Workload(3)) it pins 20 PAIR ops in a category.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "phyly_amd", "csrc")


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pairmul") / "pairmulcheck")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-I", CSRC, "-o", out, os.path.join(ROOT, "tests", "pairmulcheck_main.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


def test_pairmul_random_trees_and_config3(binary, tmp_path):
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
    tag, pairs, folded, paired = lines[0].split()
    # 20 PAIR ops a category: each removes a dispatch of the folded stream, and the shorter stream has fewer REFILLs
    assert tag == "config3" and int(pairs) == 20 and int(paired) <= int(folded) - 20
    out = lines[1].split()
    assert out[0] == "ok"
    within3, slots4, npair, adv_left, c_parity_odd, c_table, c_parity, c_swap, c_drop, c_adv, c_refill = (int(v) for v in out[1:])
    # most of the generator's trees that the streamed form takes are within 3 slots, some need 4; PAIR ops are common; every
    # negative control ran on many trees
    assert within3 >= 1500 and slots4 >= 10 and npair > within3
    # (the first observation always has a twin on the other buffer; a tree needs a second observation outside a leading PAIR
    # for the odd flip, and two requests of different tables for the table control)
    assert c_parity_odd > 1000 and c_table > 1000
    # (an even observation without a twin: TIP_SET + PUSH slot 0, the only even one of a few tiny trees)
    assert c_parity > 0.9 * within3 and c_drop == within3 and c_refill == within3 and c_swap > 500 and c_adv > 200
