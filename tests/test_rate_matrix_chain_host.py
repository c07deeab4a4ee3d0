"""Host side of arbplf-rate-matrix-deriv (no GPU): exports, validation, the loud failure without a device, the chain rule
of plk_rate_matrix_chain against central differences, and the check of the expected-value helper (tests/qgrad_cases.py)
against the oracle alone."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import GOLDEN, load_json, nonreversible_rates
from phyly_amd.engine import load_library
import qgrad_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GTRGI = os.path.join(GOLDEN, "examples", "BEAST.GTRGI", "in.json")
LD = np.longdouble


def _validate(what, doc):
    lib = load_library()
    lib.arbplf_validate_string.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    return lib.arbplf_validate_string(what.encode(), json.dumps(doc).encode())


def test_library_exports_the_new_entry_points():
    lib = load_library()
    for name in ("plk_edge_pair_sums", "plk_rate_matrix_sens", "plk_rate_matrix_chain", "plk_group_edge_pair_sums",
                 "plk_group_rate_matrix_sens", "arbplf_rate_matrix_deriv_string"):
        assert hasattr(lib, name), name


def test_validate_accepts_and_rejects():
    md = load_json(GTRGI)["model_and_data"]
    S = len(md["character_data"]) if "character_data" in md else len(md["probability_array"])
    x = {"model_and_data": md}
    ok = lambda red: _validate("rate_matrix_deriv", dict(x, site_reduction=red))
    assert ok({"aggregation": "sum"}) == 0
    assert ok({"aggregation": "avg"}) == 0
    assert ok({"aggregation": [0.5] * S}) == 0
    assert ok({"selection": [0, 2], "aggregation": "sum"}) == 0
    assert ok({"selection": [0, 2], "aggregation": [1.5, 2.0]}) == 0
    assert _validate("rate_matrix_deriv", x) != 0                                     # no site_reduction
    assert ok({"selection": [0, 1]}) != 0                                              # no aggregation
    assert ok({"aggregation": [0.5] * (S + 1)}) != 0                                   # wrong weight length
    assert _validate("rate_matrix_deriv", dict(x, site_reduction={"aggregation": "sum"}, edge_reduction={"aggregation": "sum"})) != 0
    assert _validate("rate_matrix_deriv", dict(x, site_reduction={"aggregation": "sum"}, bogus=1)) != 0
    assert _validate("rate_matrix", x) == -1


def test_no_gpu_fails_loudly():
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.is_available())"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    if r.stdout.split()[-1:] == ["True"]:
        pytest.skip("a GPU is present")
    import arbplf
    doc = load_json(GTRGI)
    doc = json.dumps({"model_and_data": doc["model_and_data"], "site_reduction": {"aggregation": "sum"}})
    with pytest.raises(RuntimeError):
        arbplf.arbplf_rate_matrix_deriv(doc)
    p = subprocess.run([os.path.join(ROOT, "phyly_amd", "csrc", "arbplf-rate-matrix-deriv")], input=doc.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode != 0 and p.stdout == b"" and b"no CPU fallback" in p.stderr


FORMS = [(div, eq) for div in (2.5, "equilibrium_exit_rate") for eq in (False, True)]


def _f(Q, divisor, eq_root, G, root):
    Qn, pi, _ = cases.normalised(Q, divisor, want_pi=eq_root)
    return np.sum(G * Qn) + (np.sum(root * pi) if eq_root else LD(0))


@pytest.mark.parametrize("k", [2, 4, 20])
@pytest.mark.parametrize("divisor,eq_root", FORMS)
def test_chain_rule_against_central_differences(k, divisor, eq_root):
    """f(Q) = <G, Qn(Q)> + <root, pi(Q)> with fixed random G and root: plk_rate_matrix_chain returns its exact gradient.
    Central differences of the long double restatement, relative step 1e-6: truncation ~ 1e-12, rounding ~ 1e-13; bound
    1e-8 max|grad|."""
    rng = np.random.default_rng(900 + k)
    Q = nonreversible_rates(k, rng, zero_frac=0.0)
    if k > 2:
        Q[0, 2] = 0.0                                                  # one zero off-diagonal entry (still irreducible)
    G = rng.standard_normal((k, k)).astype(LD)
    root = rng.standard_normal(k).astype(LD)
    rc, grad, msg = cases.product_chain(Q, divisor, 4 if eq_root else 2, G, root if eq_root else None)
    assert rc == 0, msg
    assert np.all(np.diag(grad) == 0)
    fd = np.zeros((k, k), dtype=LD)
    for i in range(k):
        for j in range(k):
            if i == j:
                continue
            h = LD(1e-6) * LD(max(Q[i, j], 1.0))
            Qp, Qm = np.array(Q, dtype=LD), np.array(Q, dtype=LD)
            Qp[i, j] += h
            Qm[i, j] -= h
            fd[i, j] = (_f(Qp, divisor, eq_root, G, root) - _f(Qm, divisor, eq_root, G, root)) / (2 * h)
    scale = float(np.max(np.abs(fd)))
    err = float(np.max(np.abs(grad.astype(LD) - fd))) / scale
    helper = float(np.max(np.abs(cases.chain(Q, divisor, eq_root, G, root) - fd))) / scale
    print("k=%d divisor=%s eq_root=%s: product %.3g, helper %.3g of max|grad|" % (k, divisor, eq_root, err, helper))
    assert err <= 1e-8 and helper <= 1e-8


def test_reducible_matrix_is_refused():
    Q = np.zeros((4, 4))
    Q[0, 1], Q[1, 0], Q[2, 3], Q[3, 2] = 1.0, 2.0, 0.5, 1.5          # two blocks
    G = np.ones((4, 4))
    for divisor, mode in (("equilibrium_exit_rate", 2), (1.0, 4), ("equilibrium_exit_rate", 4)):
        rc, _, msg = cases.product_chain(Q, divisor, mode, G, np.ones(4))
        assert rc != 0 and "rate matrix is reducible" in msg
    rc, grad, msg = cases.product_chain(Q, 1.0, 2, G, None)               # neither form needs pi
    assert rc == 0 and np.all(grad == 0)


def test_q128_images():
    lib = ctypes.CDLL("libquadmath.so.0")
    lib.quadmath_snprintf.restype = ctypes.c_int
    vals = np.array([0.0, 1.0, -2.5, 0.1, 1e-300, 3e300])
    img = cases.q128(vals).view(np.uint8).reshape(-1, 16)
    import struct
    for v, b in zip(vals, img):
        # a binary128 with the double's value: sign, exponent re-biased, the 52 mantissa bits at the top of 112
        hi = struct.unpack("<Q", bytes(b[8:]))[0]
        lo = struct.unpack("<Q", bytes(b[:8]))[0]
        if v == 0:
            assert hi == 0 and lo == 0
            continue
        e = ((hi >> 48) & 0x7FFF) - 16383
        man = ((hi & ((1 << 48) - 1)) << 64 | lo) / 2.0 ** 112
        assert (-1.0 if hi >> 63 else 1.0) * (1 + man) * 2.0 ** e == v


@pytest.fixture(scope="module")
def six_taxon(oracle):
    rng = np.random.default_rng(77)
    edges = [[0, 1], [0, 2], [1, 3], [1, 4], [2, 5], [2, 6], [5, 7], [5, 8], [6, 9], [6, 10]]
    leaves = [3, 4, 7, 8, 9, 10]
    S, k = 50, 4
    codes = np.full((S, 11), k, dtype=int)
    codes[:, leaves] = rng.integers(0, k, (S, 6))
    md = {"edges": edges, "edge_rate_coefficients": [float(v) for v in rng.uniform(0.05, 0.4, 10)],
          "rate_matrix": nonreversible_rates(k, rng, zero_frac=0.0).tolist(),
          "character_definitions": np.vstack([np.eye(k), np.ones((1, k))]).tolist(), "character_data": codes.tolist(),
          "gamma_rate_mixture": dict(gamma_shape=0.8, gamma_categories=2)}
    return md, rng.uniform(0.2, 2.0, S)


def _ll_sum(oracle, md, weights):
    m = oracle.parse_model(md)
    w = oracle.prepare(m)
    ll, _ = oracle.site_ll(m, w, B=m.B, precise=2)
    return np.sum(np.asarray(ll, dtype=LD) * np.asarray(weights, dtype=LD))


@pytest.mark.parametrize("divisor,eq_root", FORMS)
def test_helper_against_differences_of_the_oracle_ll(oracle, six_taxon, divisor, eq_root):
    """the expected-value helper (oracle G from k^2 unit directions, root from one-hot root priors, chain rule in long
    double) against Richardson-extrapolated central differences of the oracle's weighted ll sum, relative steps 1e-3 and
    5e-4: truncation O(h^4), rounding ~ 1e-16 |ll| / h ~ 1e-10; bound 1e-6 max|grad|.  Fixes signs and transpositions."""
    md0, weights = six_taxon
    md = dict(md0, rate_divisor=divisor, root_prior="equilibrium_distribution" if eq_root else [0.1, 0.2, 0.3, 0.4])
    m = oracle.parse_model(md)
    w = oracle.prepare(m)
    G = cases.oracle_G(oracle, m, w, weights)
    root = cases.oracle_root(oracle, m, w, weights) if eq_root else None
    grad = cases.chain(m.rate_matrix, divisor, eq_root, G, root)
    # the adjoint route and the factored pair sums used for large k, against the literal ones
    W = cases.oracle_W(oracle, m, w, weights)
    Wf = cases.oracle_W_factored(oracle, m, w, weights)
    assert float(np.max(np.abs(W - Wf)) / np.max(np.abs(W))) <= 1e-15
    Ga = cases.oracle_G_adjoint(oracle, m, w, W)
    adj = float(np.max(np.abs(Ga - G)) / np.max(np.abs(G)))
    k = m.k
    Q = np.array(md["rate_matrix"], dtype=float)
    fd = np.zeros((k, k), dtype=LD)

    def cd(i, j, rel):
        h = rel * Q[i, j]
        out = []
        for sgn in (1, -1):
            Qx = Q.copy()
            Qx[i, j] += sgn * h
            out.append(_ll_sum(oracle, dict(md, rate_matrix=Qx.tolist()), weights))
        return (out[0] - out[1]) / (2 * LD(h))
    for i in range(k):
        for j in range(k):
            if i != j:
                fd[i, j] = (4 * cd(i, j, 5e-4) - cd(i, j, 1e-3)) / 3
    scale = float(np.max(np.abs(fd)))
    err = float(np.max(np.abs(grad - fd))) / scale
    print("divisor=%s eq_root=%s: helper vs Richardson %.3g of max|grad| = %.3g; adjoint route vs directions %.3g" % (divisor, eq_root, err, scale, adj))
    assert err <= 1e-6
    assert adj <= 1e-13
