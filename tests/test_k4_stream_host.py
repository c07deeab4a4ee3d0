"""CPU: op words, stream layout and host replay of the streamed-code k = 4 interpreter (k_ll_fused4_v4s;
phyly_amd/csrc/plk_program.h) under AddressSanitizer + UBSan.

tests/streamcheck_main.cpp is a stand-alone program: over the seeded random trees of tests/progcheck_main.cpp it builds
the pair-table program, the streamed op words and a host image of the code stream, replays the interpreter's fetches
(every observation op must see the byte the program's op needs, for both site halves; every load must stay inside the
stream) and requires the replay check the engine runs before every launch to accept them and to refuse corrupted ones.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "phyly_amd", "csrc")


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("stream") / "streamcheck")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-I", CSRC, "-o", out, os.path.join(ROOT, "tests", "streamcheck_main.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


def test_stream_replay_random_trees(binary):
    r = subprocess.run([binary], capture_output=True, text=True, env=ENV, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    tag, trees, obs = r.stdout.split()
    # about half of the generator's trees fit the 4-slot stack and the LDS
    assert tag == "ok" and int(trees) >= 1500 and int(obs) > 100000
