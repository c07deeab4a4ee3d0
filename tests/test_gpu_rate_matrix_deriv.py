"""GPU: plk_rate_matrix_sens and arbplf-rate-matrix-deriv against the oracle-only expected values of tests/qgrad_cases.py,
against the engine's own k^2 unit directions, and the Euler identity that ties the gradient to the edge-rate derivative."""
import json
import os
import subprocess

import numpy as np
import pytest

import qgrad_cases as cases
from helpers import GOLDEN, load_json
from phyly_amd import engine as E_
from phyly_amd.engine import Engine

pytestmark = pytest.mark.gpu
LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GTRGI = os.path.join(GOLDEN, "examples", "BEAST.GTRGI", "in.json")


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _ld(x):
    return np.asarray(x[..., 0], dtype=LD) + np.asarray(x[..., 1], dtype=LD)


def _rel(got, want):
    return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))


@pytest.mark.parametrize("k,S", [(4, 257), (20, 33), (61, 33)])
def test_sens_against_oracle(eng, oracle, k, S):
    """k = 4: G from k^2 unit directions of the oracle.  k = 20, 61: k^2 binary128 Frechet matrices and up passes are out of
    reach of a test, so G comes from the oracle's W and C * E oracle Frechet matrices through the adjoint identity
    (qgrad_cases.oracle_G_adjoint, checked against the unit directions in tests/test_rate_matrix_chain_host.py)."""
    md = cases.nine_taxon_doc(S, 4, seed=40 + k) if k == 4 else cases.small_tree_doc(S, k, seed=40 + k, T=2 if k == 61 else 4)
    m, w = cases.setup_engine(eng, oracle, md)
    wt = np.random.default_rng(k).uniform(0.2, 2.0, S)
    eng.set_site_weights(wt)
    try:
        G, root = eng.rate_matrix_sens()
    finally:
        eng.set_site_weights(None)
    assert eng.info(E_.INFO_PAIR_SUMS_KERNEL) == (1 if k == 4 else 2)
    want = cases.oracle_G(oracle, m, w, wt) if k == 4 else cases.oracle_G_adjoint(oracle, m, w, cases.oracle_W_factored(oracle, m, w, wt))
    want_root = cases.oracle_root(oracle, m, w, wt)
    eg, er = _rel(_ld(G), want), _rel(_ld(root), want_root)
    print("k=%d S=%d: G %.3g of max|G|, root %.3g of max|root| (bound 1e-11)" % (k, S, eg, er))
    assert eg <= 1e-11 and er <= 1e-11


def test_sens_against_unit_directions_of_the_engine(eng, oracle):
    """the parent's route to the same numbers: 16 unit directions through plk_edge_expect_multi with
    PLK_COEF_PRIOR_RATE_EDGE, summed over edges.  A transposed G fails here."""
    md = cases.nine_taxon_doc(257, 4, seed=51)
    m, w = cases.setup_engine(eng, oracle, md)
    eng.set_site_weights(None)
    G, _ = eng.rate_matrix_sens()
    Ls = np.zeros((16, 4, 4))
    for i in range(4):
        for j in range(4):
            Ls[4 * i + j, i, j] = 1.0
    want = np.zeros((4, 4), dtype=LD)
    for b in range(4):
        _, sums = eng.edge_expect_multi(Ls[4 * b:4 * b + 4], E_.COEF_PRIOR_RATE_EDGE, per_site=False)
        want[b] = np.sum(_ld(np.asarray(sums).reshape(4, m.E, 2)), axis=1)
    err = _rel(_ld(G), want)
    print("k=4 S=257: G vs 16 unit directions of plk_edge_expect_multi %.3g of max|G| (bound 1e-11)" % err)
    assert err <= 1e-11
    assert _rel(_ld(G).T, want) > 1e-3


def _cli(doc, env=None):
    p = subprocess.run([os.path.join(ROOT, "phyly_amd", "csrc", "arbplf-rate-matrix-deriv")], input=json.dumps(doc).encode(),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **(env or {})))
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout)


def _table_err(got, rows):
    assert got["columns"] == ["first_state", "second_state", "value"]
    assert [r[:2] for r in got["data"]] == [r[:2] for r in rows]
    g = np.array([r[2] for r in got["data"]], dtype=LD)
    want = np.array([r[2] for r in rows], dtype=LD)
    return _rel(g, want)


FORMS = [(div, root) for div in (1.7, "equilibrium_exit_rate") for root in ([0.1, 0.2, 0.3, 0.4], "equilibrium_distribution")]


@pytest.mark.parametrize("divisor,root", FORMS)
def test_command_nine_taxon(oracle, divisor, root):
    import arbplf
    md = cases.nine_taxon_doc(60, 4, seed=61, divisor=divisor, root=root)
    S = 60
    wts = [float(v) for v in np.random.default_rng(3).uniform(0.0, 2.0, S)]
    for red in ({"aggregation": "sum"}, {"aggregation": "avg"}, {"aggregation": wts},
                {"selection": [3, 5, 5, 40], "aggregation": [1.0, 0.5, 2.0, 0.25]}):
        doc = {"model_and_data": md, "site_reduction": red}
        rows, _, _ = cases.expected_table(oracle, md, red)
        e_py = _table_err(json.loads(arbplf.arbplf_rate_matrix_deriv(json.dumps(doc))), rows)
        print("9 taxa divisor=%s root=%s %s: %.3g of max|value| (bound 1e-11)" % (divisor, "eq" if isinstance(root, str) else "custom", sorted(red), e_py))
        assert e_py <= 1e-11
    doc = {"model_and_data": md, "site_reduction": {"aggregation": "sum"}}
    one = _cli(doc)
    assert _table_err(one, cases.expected_table(oracle, md, {"aggregation": "sum"})[0]) <= 1e-11
    two = _cli(doc, env={"ARBPLF_DEVICES": "0,0"})
    assert _table_err(two, one["data"]) <= 1e-13


def test_command_beast_gtrgi(oracle):
    import arbplf
    md = load_json(GTRGI)["model_and_data"]
    for red in ({"aggregation": "sum"}, {"selection": [0, 1, 2, 3], "aggregation": "avg"}):
        rows, _, _ = cases.expected_table(oracle, md, red)
        err = _table_err(json.loads(arbplf.arbplf_rate_matrix_deriv(json.dumps({"model_and_data": md, "site_reduction": red}))), rows)
        print("BEAST.GTRGI %s: %.3g of max|value| (bound 1e-11)" % (sorted(red), err))
        assert err <= 1e-11


def test_euler_identity(eng, oracle):
    """with a numeric divisor, scaling Q is scaling every edge rate: sum_ij q_ij grad_ij = sum_e t_e (deriv sum)_e"""
    md = cases.nine_taxon_doc(257, 4, seed=81, divisor=2.0, root=[0.4, 0.3, 0.2, 0.1])
    m, w = cases.setup_engine(eng, oracle, md)
    eng.set_site_weights(None)
    G, _ = eng.rate_matrix_sens()
    rc, grad, msg = cases.product_chain(m.rate_matrix, 2.0, 2, _ld(G), None)
    assert rc == 0, msg
    Q = np.array(m.rate_matrix, dtype=LD)
    np.fill_diagonal(Q, 0)
    lhs = np.sum(Q * grad.astype(LD))
    _, dsum = eng.deriv(per_site=False)
    rhs = np.sum(np.asarray(m.edge_rates_csr, dtype=LD) * _ld(dsum))
    err = float(abs(lhs - rhs) / abs(rhs))
    print("Euler identity: %.3g relative (bound 1e-10)" % err)
    assert err <= 1e-10
