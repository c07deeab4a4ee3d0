"""CPU: plk_mix_term (phyly_amd/csrc/plk_mix.h), the branch-free form in which the streamed k = 4 kernel adds a category's term to
a site's scaled mixture sum, under AddressSanitizer + UBSan.

tests/mixcheck_main.cpp is a stand-alone program: it compares the function, on the uint64 view of the sum, with a verbatim copy
of the three-way form it replaced (first term / larger exponent / otherwise) over random sequences, all categories zero, a zero
term first / in the middle / last, ascending and descending exponents, exponent gaps of +-2100 and beyond, and denormal terms,
and it runs three deliberately wrong variants over the same sequences.  The two ldexp swapped and a sentinel treated as a term
must each differ somewhere.  `>=` for `>` cannot differ from the reference (equal exponents: both distances are zero and either
branch adds the same operands in the same order), so the program requires that it never does.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "phyly_amd", "csrc")


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("mixcheck") / "mixcheck")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-I", CSRC, "-o", out, os.path.join(ROOT, "tests", "mixcheck_main.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


def test_mix_term_has_the_bits_of_the_three_way_form(binary):
    r = subprocess.run([binary], capture_output=True, text=True, env=ENV, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    last = [ln for ln in r.stdout.split("\n") if ln.startswith("ok ")][0].split()
    seqs, terms, swapped, ge, sentinel = (int(v) for v in last[1:])
    assert seqs > 45000 and terms > 4 * 45000 // 2
    assert swapped > 0 and sentinel > 0 and ge == 0
