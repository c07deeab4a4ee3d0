"""CPU: the sequence that derives the formats the streamed k = 4 kernel runs (plk_k4_stream in phyly_amd/csrc/plk_program.h:
tables and category groups, the folded and the pair-product stream, the fall-backs between them, the barrier) under
AddressSanitizer + UBSan.

tests/streamformatscheck_main.cpp is a stand-alone program: over small trees that reach every branch and the tree of BASELINE
config 3 (written here from synth.Workload(3)), a grid of nchar, categories, site counts, CU counts and PLK_OPT_PAIR_TABLES
values, and the combinations of the four capabilities the engine may lack (the held-chunks, pair-product and category-group
instantiations, room for the partial sums), it requires the formats named as running to replay, the consistency the launch
relies on, a missing capability to give what the matching option bit gives, and each of six outcomes to occur.

PARENT holds, per tree, a 64-bit FNV-1a hash over all cases with every capability given: the words that run, the lists of the
pair-table format that runs, obs_row, chunks, first_y, the LDS, sync and the four info words.  The values were printed by the
same driver built against commit 3c500afd002b ("k = 4 streamed ll: no barrier in one-category phases; plan re-fitted"), the
last one in which the engine's upload_formats_fused4 held this sequence itself, with those lines of the engine copied behind
plk_k4_stream's interface: what the function derives is what the engine derived.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "phyly_amd", "csrc")

PARENT = {
    "three": "dbe7a988d9c74303",
    "four": "5077f3ef7f79aa27",
    "tip_mul": "9600aa421f840f87",
    "matvec": "fb4c095fb9354613",
    "push": "701a835fae6e5103",
    "popmul": "c3cb10c4b1725ea3",
    "slots4": "846433d430436207",
    "cat40": "b746c522a0dd8293",
    "config3": "1c28b14041da3faf",
}


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("streamformats") / "streamformatscheck")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-I", CSRC, "-o", out, os.path.join(ROOT, "tests", "streamformatscheck_main.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


def test_stream_formats_sequence(binary, tmp_path):
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
    hashes = dict(ln.split()[1:] for ln in lines if ln.startswith("hash "))
    assert hashes == PARENT
    last = [ln for ln in lines if ln.startswith("ok ")][0].split()
    cases, outcomes = int(last[1]), [int(v) for v in last[2:]]
    # checked, folded, pair-product words; tables in one group, in several; the plan's groups taken back
    assert cases > 10000 and len(outcomes) == 6 and all(n > 0 for n in outcomes), outcomes
