"""CPU: the barrier default of the streamed k = 4 kernel (plk_v4s_auto_sync and the sync that plk_k4_stream decides on the
formats that run, phyly_amd/csrc/plk_program.h) under AddressSanitizer + UBSan.

tests/synccheck_main.cpp is a stand-alone program: on the tree of BASELINE config 3 (written here from synth.Workload(3)) it
asks for the plan of several (categories, sites, CUs) and what runs under it, and requires the waves to meet before every category unless one
category is resident at a time and its matrix stream and op words fit the scalar cache, the option bits to force either, and
config 3 itself, and the same alignment cut for 8 GPUs, to run without the barrier while plans below the gate keep it.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "phyly_amd", "csrc")


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("sync") / "synccheck")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-I", CSRC, "-o", out, os.path.join(ROOT, "tests", "synccheck_main.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


def test_sync_default_follows_the_plan(binary, tmp_path):
    from phyly_amd import synth
    wl = synth.Workload(3)
    assert wl.nchar == 5
    tree = tmp_path / "config3.tree"
    with open(tree, "w") as f:
        f.write("%d\n" % wl.N)
        for arr in (wl.indptr, wl.indices, wl.preorder):
            f.write(" ".join(str(int(v)) for v in arr) + "\n")
    r = subprocess.run([binary, str(tree)], capture_output=True, text=True, env=ENV, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    tag, without, with_barrier = r.stdout.split()
    assert tag == "ok" and int(without) >= 6 and int(with_barrier) >= 3
