"""CPU: the host-only check of the values K1 is given (phyly_amd/csrc/plk_k1_check.h) and the squaring count that
replaced the device loop, under AddressSanitizer + UBSan in a stand-alone program (tests/k1_args_main.c), and the same
cases through plk_check_model_values of the loaded library, which needs no engine and no GPU.

Cases (tests/k1_cases.check_cases): inf, -inf and NaN in every array, negative rates and priors, -0.0 (accepted), the last
accepted and the first refused value at r_c t_e |Qn|_inf = 2^40, products that overflow (1e308 x 2, 1e200 x 1e200, a
normalised matrix scaled by 1e300), k = 1 and k = 64, C = 64, E = 1; the root prior is read only in the modes that use it.
The squaring count equals that of the loop `while (norm > 2^-5) { norm /= 2; sq++; }` at every power of two of the double
range, its two neighbours and three random mantissas per exponent, and is PLK_K1_MAX_SQ for an infinite norm."""
import os
import subprocess

import pytest

import k1_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "phyly_amd", "csrc")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
CASES = K.check_cases()


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("k1args") / "k1_args")
    cmd = ["gcc", "-O1", "-g", "-std=c99", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-I", CSRC, "-o", out, os.path.join(ROOT, "tests", "k1_args_main.c"), "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


def test_cases_cover_what_the_check_refuses():
    names = [c[0] for c in CASES]
    assert len(set(names)) == len(names)
    assert sum(1 for c in CASES if c[1]) >= 30 and sum(1 for c in CASES if not c[1]) >= 10
    assert {len(c[2]["Qn"]) for c in CASES} >= {1, 3, 64} and {len(c[2]["cr"]) for c in CASES} >= {1, 64}


def test_squaring_count_equals_the_loop(binary):
    r = subprocess.run([binary], capture_output=True, text=True, env=ENV, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    tag, norms = r.stdout.split()
    assert tag == "ok" and int(norms) >= 12000


def test_check_under_sanitizers(binary, tmp_path):
    f = tmp_path / "cases.txt"
    f.write_text("\n".join(K.check_case_line(name, v) for name, _, v, _ in CASES) + "\n")
    r = subprocess.run([binary, str(f)], capture_output=True, text=True, env=ENV, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(CASES)
    for line, (name, refused, _, names) in zip(lines, CASES):
        got_name, rc, msg = (line.split(" ", 2) + [""])[:3]
        assert got_name == name
        assert (int(rc) != 0) == refused, line
        assert bool(msg) == refused, line
        if names is not None:
            assert "edge %d " % names[0] in msg and "category %d " % names[1] in msg, line


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_library_export(name):
    from phyly_amd import engine
    _, refused, v, _ = next(c for c in CASES if c[0] == name)
    rc = engine.check_model_values(v["Qn"], v["er"], v["cr"], v["cp"], v["root_mode"], v["rw"], Qn_lo=v["Qn_lo"])
    assert rc == (engine.E_ARG if refused else 0)


def test_library_export_argument_errors():
    from phyly_amd import engine
    v = K.check_cases()[0][2]
    assert engine.check_model_values(v["Qn"], v["er"], v["cr"], v["cp"], 2, None) == engine.E_ARG          # root_w required
    assert engine.check_model_values(v["Qn"], v["er"], v["cr"], v["cp"], 7, v["rw"]) == engine.E_ARG       # no such root mode
