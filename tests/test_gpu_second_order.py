"""GPU: plk_second_order on the k = 4 second-order pass (plk_hess4.h) and the three commands built on it
(arbplf-inv-hess, arbplf-newton-delta, arbplf-newton-update).

Bars: Hessian <= 1e-11 * max|H| against the binary128 oracle (the bar of test_gpu_hess.py), gradient sums <= 1e-12 of the
largest entry (test_gpu_deriv_marginal.py).  The commands are compared with an extended-precision solve, done here, of
the ORACLE's Hessian and gradient: with the product's Hessian good to 1e-11 * ||H||_inf per entry the first-order
perturbation bound is |got - want|_max <= 2 * kappa * E * 1e-11 * |want|_max, kappa = cond_inf of the oracle's Hessian
(the factor 2 covers the gradient's own error and the second-order term while kappa * E * 1e-11 <= 0.1).  A case counts
only if kappa * E * 1e-11 <= 1e-6; above that it is checked for "refused or finite"."""
import copy
import json
import os
import random
import subprocess

import numpy as np
import pytest

from helpers import GOLDEN, load_json, oracle_model
from phyly_amd import engine as E_
from phyly_amd import synth
import second_order_cases as cases
from second_order_cases import reference_solve as _reference

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HESS = os.path.join(GOLDEN, "examples", "Felsenstein.2004.fig.16.4", "hess")
K4_SECOND_ORDER, GENERIC = 5, 2
COMMANDS = ("inv_hess", "newton_delta", "newton_update")
# Under a reversible model with the stationary root prior only the SUM of the two root edges is identifiable (pulley
# principle): the Hessian is singular there and the commands refuse it.  The command tests on synthetic trees therefore
# put a non-stationary prior at the root.
ROOT_W = [0.4, 0.3, 0.2, 0.1]


def _json_model(w, codes):
    md = w.json_model(codes)
    md["root_prior"] = ROOT_W
    return md


@pytest.fixture(scope="module")
def eng():
    e = E_.Engine(0)
    yield e
    e.close()


def _with_tree(w, edges):
    """a synth.Workload on a tree given as [[parent, child], ...]"""
    w.edges = edges
    w.E = len(edges)
    w.N = w.E + 1
    w.edge_rates = synth.branch_lengths(w.E, w.seed)
    w.indptr, w.indices, w.preorder, w.order = synth.csr_from_edges(edges)
    w.edge_rates_csr = np.zeros(w.E)
    for i, pos in enumerate(w.order):
        w.edge_rates_csr[pos] = w.edge_rates[i]
    w._cum = None
    return w


def _caterpillar(T):
    edges, top = [[T, 0], [T, 1]], T
    for leaf in range(2, T):
        edges += [[top + 1, top], [top + 1, leaf]]
        top += 1
    return edges


def _oracle_sums(oracle, w, codes, wts, defs=None):
    defs = w.defs if defs is None else defs
    m, ow = oracle_model(oracle, w, codes)
    B = defs[codes.T]
    wl = wts[:, None].astype(np.longdouble)
    H = (oracle.site_hess(m, ow, B, precise=2).astype(np.longdouble) * wl[:, :, None]).sum(axis=0).astype(float)
    g = (oracle.site_deriv(m, ow, B, precise=2).astype(np.longdouble) * wl).sum(axis=0).astype(float)
    return g, H


def _check_engine(eng, oracle, w, codes, wts=None, defs=None):
    w.setup_engine(eng)
    eng.set_patterns_codes(codes, w.defs if defs is None else defs)
    S = codes.shape[1]
    wts = np.ones(S) if wts is None else wts
    eng.set_site_weights(wts)
    g, H = eng.second_order()
    eng.set_site_weights(None)
    assert eng.info(E_.INFO_UPDOWN_KERNEL) == K4_SECOND_ORDER      # the new pass ran, not the generic one
    gw, Hw = _oracle_sums(oracle, w, codes, wts, defs)
    eh = np.max(np.abs(H - Hw)) / np.max(np.abs(Hw))
    eg = np.max(np.abs(g - gw)) / np.max(np.abs(gw))
    print("%s E=%d S=%d: hess err %.3g grad err %.3g" % (w.name, w.E, S, eh, eg))
    assert np.array_equal(H, H.T)
    assert eh <= 1e-11, eh
    assert eg <= 1e-12, eg


@pytest.mark.parametrize("T,model,S,missing", [(10, "gtr_g4", 60, 0.0), (40, "gtr_g4", 24, 0.0), (12, "hky85", 40, 0.0),
                                                (14, "gtr_g4", 30, 0.2)])
def test_kernel_matches_oracle(eng, oracle, T, model, S, missing):
    w = synth.Workload(T=T, k=4, tree="yule", model=model, seed=21)
    codes = w.random_codes(S, seed=3, missing_frac=missing) if missing else w.simulate(S)
    _check_engine(eng, oracle, w, codes, np.linspace(0.5, 1.5, S))


def test_rescaled_nodes(eng, oracle):
    """Observations scaled so that the site likelihoods leave the double range (~1e-990), at the bar the existing
    tiny-likelihood test of test_gpu_hess.py uses for exactly this input, 1e-10.  This is an extra case: the issue's "tree
    deep enough to need rescaled nodes" at 1e-11 is the T = 40 case of test_kernel_matches_oracle (the traversal program
    rescales a node every 16 accumulated edges, so that tree has rescaled nodes)."""
    w = synth.Workload(T=64, k=4, tree="yule", model="gtr_g4", seed=33)
    codes = w.simulate(4)
    defs = w.defs.copy()
    defs[:4] *= 1e-15
    w.setup_engine(eng)
    eng.set_patterns_codes(codes, defs)
    g, H = eng.second_order()
    assert eng.info(E_.INFO_UPDOWN_KERNEL) == K4_SECOND_ORDER
    gw, Hw = _oracle_sums(oracle, w, codes, np.ones(4), defs)
    assert np.all(np.isfinite(H))
    assert np.max(np.abs(H - Hw)) <= 1e-10 * np.max(np.abs(Hw))        # the bar of test_rescaled_passes_tiny_likelihoods
    assert np.max(np.abs(g - gw)) <= 1e-12 * np.max(np.abs(gw))


@pytest.mark.parametrize("name,edges,model", [
    ("E=1 (one launch of one model)", [[1, 0]], "hky85"),
    ("E=2 (one launch of two)", [[2, 0], [2, 1]], "gtr_g4"),
    ("3-taxon star, E=3 (a launch of four with an idle row)", [[3, 0], [3, 1], [3, 2]], "gtr_g4"),
    ("E=4", [[3, 0], [3, 1], [4, 3], [4, 2]], "hky85"),
    ("E=5: four + one", [[3, 0], [3, 1], [4, 3], [4, 2], [5, 4]], "gtr_g4"),
    ("caterpillar of 8, E=14: four x 3 + two", _caterpillar(8), "gtr_g4"),
    ("caterpillar of 5 under one category, E=8", _caterpillar(5), "hky85"),
])
def test_every_instantiation(eng, oracle, name, edges, model):
    """NM = 1, 2 and 4 models per launch, last launches with fewer rows, C = 1 (hky85) and C = 4 (gtr_g4)"""
    w = _with_tree(synth.Workload(T=3, k=4, tree="yule", model=model, seed=5), edges)
    w.name = name
    codes = w.random_codes(25, seed=8, missing_frac=0.1)
    if w.E == 1:        # one leaf under an unobserved root says nothing about the edge: observe the root as well
        codes[w.preorder[0]] = (codes[w.indices[0]] + np.arange(25)) % 4
    _check_engine(eng, oracle, w, codes, np.linspace(0.25, 2.0, 25))


@pytest.mark.parametrize("S", [60, 20000])
def test_ab_against_the_generic_passes(eng, S):
    """both paths are within 1e-11 of the exact Hessian, so within 2e-11 * max|H| of each other"""
    w = synth.Workload(T=24, k=4, tree="yule", model="gtr_g4", seed=9)
    w.setup_engine(eng)
    eng.set_patterns_codes(w.simulate(S), w.defs)
    eng.set_option(E_.OPT_FORCE_GENERIC, 1)
    g1, H1 = eng.second_order()
    k1 = eng.info(E_.INFO_UPDOWN_KERNEL)
    eng.set_option(E_.OPT_FORCE_GENERIC, 0)
    g0, H0 = eng.second_order()
    k0 = eng.info(E_.INFO_UPDOWN_KERNEL)
    assert (k1, k0) == (GENERIC, K4_SECOND_ORDER)
    dh = np.max(np.abs(H1 - H0)) / np.max(np.abs(H0))
    dg = np.max(np.abs(g1 - g0)) / np.max(np.abs(g0))
    assert dh <= 2e-11 and dg <= 2e-12, "largest difference: Hessian %.3g, gradient %.3g of the largest entry" % (dh, dg)


def test_hess_is_second_order_without_gradient(eng):
    w = synth.Workload(T=10, k=4, tree="yule", model="gtr_g4", seed=2)
    w.setup_engine(eng)
    eng.set_patterns_codes(w.simulate(300), w.defs)
    wts = np.linspace(0.1, 3.0, 300)
    eng.set_site_weights(wts)
    H = eng.hess()
    out = np.zeros((w.E, w.E, 2))
    eng._check(eng._lib.plk_second_order(eng._h, None, out.ctypes.data))
    g, H2 = eng.second_order()
    _, s = eng.deriv(per_site=False)
    eng.set_site_weights(None)
    assert np.array_equal(H, out[..., 0] + out[..., 1]) and np.array_equal(H, H2)
    d = s[:, 0] + s[:, 1]
    assert np.max(np.abs(g - d)) <= 1e-13 * np.max(np.abs(d))


# ------------------------------------------------------------------ the three commands

def _table(s):
    return json.loads(s)


def _fn(name):
    import arbplf
    return getattr(arbplf, "arbplf_" + name)


_check_commands = cases.check_commands       # shared with test_gpu_second_order_families.py


@pytest.mark.parametrize("d", ["with.full.data", "with.leaf.data"])
def test_commands_on_reference_inputs(oracle, d):
    assert _check_commands(oracle, load_json(os.path.join(HESS, d, "in.json")))


def test_commands_on_random_inputs(oracle):
    """20 seeded random_model documents, made regular by second_order_cases.regular_document (its docstring says why and
    how); at most a quarter may fall above the condition kappa * E * 1e-11 <= 1e-6.  The same share is asserted without a
    GPU, from the oracle alone, in test_second_order_host.py."""
    counted = sum(bool(_check_commands(oracle, x)) for x in cases.random_documents())
    assert counted >= 15, "only %d of %d random cases were conditioned well enough to count" % (counted, cases.CASES)


def test_consistency_of_the_three_commands():
    x = load_json(os.path.join(HESS, "with.full.data", "in.json"))
    s = json.dumps(x)
    r = np.array(x["model_and_data"]["edge_rate_coefficients"])
    E = len(r)
    delta = np.array([v[-1] for v in _table(_fn("newton_delta")(s))["data"]])
    upd = np.array([v[-1] for v in _table(_fn("newton_update")(s))["data"]])
    assert np.all(np.abs((upd - r) - delta) <= np.spacing(np.maximum(np.abs(upd), np.abs(r))))
    inv = np.array([v[-1] for v in _table(_fn("inv_hess")(s))["data"]]).reshape(E, E)
    import arbplf
    H = np.array([v[-1] for v in _table(arbplf.arbplf_hess(s))["data"]]).reshape(E, E)
    assert np.array_equal(inv, inv.T)
    kappa = np.max(np.sum(np.abs(H), axis=1)) * np.max(np.sum(np.abs(inv), axis=1))
    resid = np.max(np.abs(H.astype(np.longdouble) @ inv.astype(np.longdouble) - np.eye(E)))
    assert resid <= kappa * E * 2e-11, (resid, kappa)


def test_site_weights_equal_duplicated_sites():
    """test_scripts/test_site_weights.py of the reference, restated: integer weights against repeated columns"""
    w = synth.Workload(T=7, k=4, tree="yule", model="gtr_g4", seed=12)
    codes = w.simulate(40)
    reps = np.array([1 + (i % 3) for i in range(40)])
    xa = {"model_and_data": _json_model(w, codes), "site_reduction": {"aggregation": reps.tolist()}}
    xb = {"model_and_data": _json_model(w, np.repeat(codes, reps, axis=1)), "site_reduction": {"aggregation": "sum"}}
    import arbplf
    H = np.array([v[-1] for v in _table(arbplf.arbplf_hess(json.dumps(xa)))["data"]]).reshape(w.E, w.E)
    kappa = np.max(np.sum(np.abs(H), axis=1)) * np.max(np.sum(np.abs(np.linalg.inv(H)), axis=1))
    assert kappa * w.E * 1e-11 <= 1e-6
    for name in COMMANDS:
        a = np.array([v[-1] for v in _table(_fn(name)(json.dumps(xa)))["data"]])
        b = np.array([v[-1] for v in _table(_fn(name)(json.dumps(xb)))["data"]])
        ref = np.max(np.abs(a)) if name != "newton_update" else np.max(np.abs(a - np.array(w.edge_rates)))
        assert np.max(np.abs(a - b)) <= 2 * kappa * w.E * 1e-11 * ref, name


# ------------------------------------------------------------------ the reference's invariance scripts, restated
# Each pair is two evaluations of the same quantity, so the kappa-scaled bar applies; kappa from the product's Hessian of
# the first document, and the pair must be inside the range where the bound is valid (kappa * E * 1e-11 <= 0.1).

def _values(name, x):
    return np.array([v[-1] for v in _table(_fn(name)(json.dumps(x)))["data"]])


def _check_pair(xa, xb):
    import arbplf
    r = np.array(xa["model_and_data"]["edge_rate_coefficients"], dtype=float)
    E = len(r)
    H = np.array([v[-1] for v in _table(arbplf.arbplf_hess(json.dumps(xa)))["data"]]).reshape(E, E)
    kappa = cases.cond_inf(H, np.linalg.inv(H))
    assert kappa * E * 1e-11 <= 0.1, kappa
    for name in COMMANDS:
        a, b = _values(name, xa), _values(name, xb)
        scale = np.max(np.abs(a - r)) if name == "newton_update" else np.max(np.abs(a))
        err = np.max(np.abs(a - b))
        assert err <= 2 * kappa * E * 1e-11 * scale, (name, err, kappa, scale)


_RD_PA = [[[0.25, 0.75]] + [[1, 0] if b == "0" else [0, 1] for b in bits]
          for bits in ("000", "100", "010", "001", "111", "011", "101", "110")]


def _rate_divisor_doc(Q, divisor, coefficients=(2, 13, 19)):
    return {"model_and_data": {"edges": [[0, 1], [0, 2], [0, 3]], "edge_rate_coefficients": list(coefficients),
                               "rate_matrix": Q, "rate_divisor": divisor, "probability_array": copy.deepcopy(_RD_PA)},
            "site_reduction": {"aggregation": [10, 1, 2, 3, 20, 2, 5, 7]}}


def _root(x, row, prior=None):
    for site in x["model_and_data"]["probability_array"]:
        site[0] = list(row)
    if prior is not None:
        x["model_and_data"]["root_prior"] = prior
    return x


def test_rate_divisor_scaling():
    """test_scripts/test_rate_divisor.py: Q / 100 = 3Q / 300; a numeric divisor against equilibrium_exit_rate (1.5 for this
    matrix), with the root observation, with the explicit and with the stationary root prior"""
    A, B = [[0, 3], [1, 0]], [[0, 9], [3, 0]]
    small = [c / 100 for c in (2, 13, 19)]
    _check_pair(_rate_divisor_doc(A, 100), _rate_divisor_doc(B, 300))
    _check_pair(_rate_divisor_doc(A, 1.5, small), _rate_divisor_doc(B, "equilibrium_exit_rate", small))
    _check_pair(_root(_rate_divisor_doc(A, 1.5, small), [1, 1], [0.25, 0.75]),
                _root(_rate_divisor_doc(B, "equilibrium_exit_rate", small), [1, 1], "equilibrium_distribution"))
    _check_pair(_root(_rate_divisor_doc(A, 1.5, small), [1, 1], "equilibrium_distribution"),
                _root(_rate_divisor_doc(B, "equilibrium_exit_rate", small), [1, 1], [0.25, 0.75]))
    C = _root(_rate_divisor_doc(A, 100), [1, 1], "equilibrium_distribution")       # diagonal entries are ignored
    D = copy.deepcopy(C)
    for i in range(2):
        D["model_and_data"]["rate_matrix"][i][i] = 42
    _check_pair(C, D)


def test_root_prior_spellings():
    """test_scripts/test_root_prior.py: the stationary distribution (0.25, 0.75) as root_prior keyword, as an observation
    row at the root, and as an explicit root_prior list"""
    A, B = [[0, 3], [1, 0]], [[0, 9], [3, 0]]
    eq = _root(_rate_divisor_doc(A, 100), [1, 1], "equilibrium_distribution")
    _check_pair(eq, _root(_rate_divisor_doc(B, 300), [0.25, 0.75]))
    _check_pair(eq, _root(_rate_divisor_doc(B, 300), [1, 1], [0.25, 0.75]))


def _seven_edge_doc(root_row, root_prior=None):
    obs = lambda i: [1.0 if j == i else 0.0 for j in range(4)]
    site = lambda third: [obs(0), obs(1), obs(third), obs(1), obs(2), list(root_row), [1] * 4, [1] * 4]
    md = {"edges": [[5, 0], [5, 1], [5, 6], [6, 2], [6, 7], [7, 3], [7, 4]],
          "edge_rate_coefficients": [0.01, 0.2, 0.15, 0.3, 0.05, 0.3, 0.02],
          "rate_matrix": [[0, .3, .4, .5], [.3, 0, .3, .3], [.3, .6, 0, .3], [.3, .3, .3, 0]],
          "probability_array": [site(1), site(3)]}
    if root_prior is not None:
        md["root_prior"] = root_prior
    return {"model_and_data": md, "site_reduction": {"aggregation": "sum"}}


@pytest.mark.parametrize("gamma,mixture", [
    ({"gamma_shape": 0.5, "gamma_categories": 4},
     {"rates": [0.0333877533835995, 0.251915917593438, 0.820268481973649, 2.89442784704931], "prior": "uniform_distribution"}),
    ({"gamma_shape": 0.5, "gamma_categories": 4, "invariable_prior": 0.3},
     {"rates": [0.0333877533835995 / 0.7, 0.251915917593438 / 0.7, 0.820268481973649 / 0.7, 2.89442784704931 / 0.7, 0.0],
      "prior": [0.7 / 4, 0.7 / 4, 0.7 / 4, 0.7 / 4, 0.3]}),
])
def test_gamma_discretisation_equals_explicit_mixture(gamma, mixture):
    """test_scripts/test_gamma_discretization.py.  The script's rates are printed to 15 digits, so the two documents differ
    by 1e-15 relative in the rates themselves: far inside the bar"""
    xa, xb = _seven_edge_doc([1] * 4, "uniform_distribution"), _seven_edge_doc([1] * 4, "uniform_distribution")
    xa["model_and_data"]["gamma_rate_mixture"] = gamma
    xb["model_and_data"]["rate_mixture"] = mixture
    _check_pair(xa, xb)


def test_rate_mixture_equals_block_diagonal_matrix():
    """test_scripts/test_rate_mixture_vs_block.py: rates (1, 2) with prior (0.25, 0.75) against an 8-state block-diagonal
    matrix whose second block is twice the first, the prior in the root's observation row"""
    xa = _seven_edge_doc([0.25] * 4)
    xa["model_and_data"]["rate_mixture"] = {"rates": [1, 2], "prior": [0.25, 0.75]}
    xb = _seven_edge_doc([0.25] * 4)
    m = xb["model_and_data"]
    Q = m["rate_matrix"]
    m["rate_matrix"] = [Q[i] + [0.0] * 4 for i in range(4)] + [[0.0] * 4 + [2 * v for v in Q[i]] for i in range(4)]
    m["probability_array"] = [[row + row if row != [0.25] * 4 else [0.0625] * 4 + [0.1875] * 4 for row in site]
                              for site in m["probability_array"]]
    _check_pair(xa, xb)


def test_newton_converges(eng):
    w = synth.Workload(T=12, k=4, tree="yule", model="gtr_g4", seed=6)
    k0 = w.prepare()
    eng.set_tree(w.indptr, w.indices, w.preorder)
    eng.set_model(k0["Qn"], w.edge_rates_csr, k0["cat_rates"], k0["cat_prior"], E_.ROOT_CUSTOM, np.array(ROOT_W), Qn_lo=k0["Qn_lo"])
    codes = w.simulate(20000)
    eng.set_patterns_codes(codes, w.defs)
    fit = eng.fit_edge_rates(w.edge_rates_csr.copy(), method=E_.FIT_LBFGS, max_iter=400, ftol=1e-14)
    opt = np.asarray(fit[0] if isinstance(fit, tuple) else fit, dtype=float)
    inv_order = np.array(w.order)
    rates = (opt * 1.02)[inv_order]                      # user edge order
    md = _json_model(w, codes)
    norms = []
    for _ in range(6):
        md["edge_rate_coefficients"] = rates.tolist()
        s = json.dumps({"model_and_data": md, "site_reduction": {"aggregation": "sum"}})
        norms.append(max(abs(v[-1]) for v in _table(_fn("newton_delta")(s))["data"]))
        if len(norms) == 6:
            break
        rates = np.array([v[-1] for v in _table(_fn("newton_update")(s))["data"]])
    print("newton delta norms:", norms)
    assert all(b < a for a, b in zip(norms[:4], norms[1:5])), norms     # falls at every step until the noise floor
    assert norms[5] <= 1e-8 * np.max(rates), norms
    csr = np.zeros(w.E)
    csr[inv_order] = rates
    em = eng.fit_edge_rates(csr.copy(), method=E_.FIT_EM, max_iter=400, ftol=0.0)
    em = np.asarray(em[0] if isinstance(em, tuple) else em, dtype=float)
    assert np.max(np.abs(em - csr) / csr) <= 1e-6
    eng.update_edge_rates(w.edge_rates_csr)


def test_refusals(capfd):
    import arbplf
    with open(os.path.join(HESS, "with.no.data", "in.json")) as f:
        nodata = f.read()
    for name in COMMANDS:
        with pytest.raises(RuntimeError):
            _fn(name)(nodata)
        assert "singular to working precision" in capfd.readouterr().err
    x = load_json(os.path.join(HESS, "with.leaf.data", "in.json"))
    for bad in ({k: v for k, v in x.items() if k != "site_reduction"},
                dict(x, site_reduction={"selection": [0]}),
                dict(x, edge_reduction={"aggregation": "sum"})):
        for name in COMMANDS:
            with pytest.raises(RuntimeError):
                _fn(name)(json.dumps(bad))
    with pytest.raises(RuntimeError):
        arbplf.arbplf_newton_refine(json.dumps(x))
    r = subprocess.run([os.path.join(ROOT, "phyly_amd", "csrc", "arbplf-newton-delta")], input=nodata, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "singular to working precision" in r.stderr and r.stdout.strip() == ""


@pytest.mark.parametrize("name", COMMANDS)
def test_cli(name):
    path = os.path.join(HESS, "with.leaf.data", "in.json")
    with open(path) as f:
        want = _fn(name)(f.read())
    with open(path) as f:
        r = subprocess.run([os.path.join(ROOT, "phyly_amd", "csrc", "arbplf-" + name.replace("_", "-"))], stdin=f, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == want.strip() and json.loads(r.stdout)


@pytest.mark.parametrize("name", COMMANDS)
def test_group_path(monkeypatch, name):
    w = synth.Workload(T=9, k=4, tree="yule", model="gtr_g4", seed=21)
    s = json.dumps({"model_and_data": _json_model(w, w.simulate(400)), "site_reduction": {"aggregation": "sum"}})
    monkeypatch.delenv("ARBPLF_DEVICES", raising=False)
    one = _table(_fn(name)(s))
    monkeypatch.setenv("ARBPLF_DEVICES", "0,0")
    two = _table(_fn(name)(s))
    monkeypatch.delenv("ARBPLF_DEVICES", raising=False)
    a, b = np.array([v[-1] for v in one["data"]]), np.array([v[-1] for v in two["data"]])
    import arbplf
    E = w.E
    H = np.array([v[-1] for v in _table(arbplf.arbplf_hess(s))["data"]]).reshape(E, E)
    kappa = np.max(np.sum(np.abs(H), axis=1)) * np.max(np.sum(np.abs(np.linalg.inv(H)), axis=1))
    # the two-engine sums differ from one engine's by 1e-14 relative (test_gpu_group.py); through the solve: kappa * E times that
    assert np.max(np.abs(a - b)) <= kappa * E * 1e-14 * max(np.max(np.abs(a)), 1e-3)
