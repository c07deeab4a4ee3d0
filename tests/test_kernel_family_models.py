"""CPU only: the models of tests/test_gpu_kernel_families.py can tell a wrong kernel from a right one.

For every state count there, the oracle alone shows that a plausible kernel bug moves the per-site log likelihood by far
more than the 1e-12 tolerance of the GPU tests: P read transposed, uniform root weights (or, for a uniform root prior,
the equilibrium ones: root modes mixed up), the matrices of two rate categories swapped on one edge (a stride mistake),
every category given category 0's matrices.  Also pinned: why the BASELINE models were blind to all of these (symmetric
Q, uniform pi, symmetric P, one rate category).

The same for the k = 4 models of tests/test_gpu_k4_variants.py (helpers.K4_MODELS), with two more bugs: the category
priors permuted, and the two leaf codes of a cherry swapped (a pair table read as [code_c][code_b]); and what the gtr_g4
workload of the other k = 4 tests could not see."""
import copy

import numpy as np
import pytest

from helpers import FAMILY_MODELS, IRREGULAR_CHERRY, K4_MODELS, cherry_with_unequal_edges, family_workload, k4_workload, oracle_model

TEETH = 1e-6        # a bug must move some site's ll by this much (relative to max(1, |ll|)), >> the 1e-12 GPU tolerance


def _ll(oracle, m, w, codes, defs):
    ll, _ = oracle.site_ll(m, w, codes=np.ascontiguousarray(codes.T), defs=defs, precise=1)   # precise=1 reads w["P"]
    return ll


def _moved(a, b):
    return np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))


def _bugs(wl, m, w):
    """{name: (model, workspace)} of the kernel bugs that apply to a model with w["C"] categories"""
    k, C, E, P = wl.k, w["C"], wl.E, w["P"]
    bugs = {}
    bugs["P transposed"] = (m, dict(w, P=np.ascontiguousarray(P.transpose(0, 1, 3, 2))))
    mu = copy.copy(m)
    mu.root_mode = 2                                     # custom weights
    if wl.root == "uniform":
        rw = w["pi"].copy()                              # uniform <-> equilibrium mixed up
    else:
        rw = np.full(k, 1.0 / k)
    bugs["root weights"] = (mu, dict(w, root_w=rw))
    if C > 1:
        # one edge only: swapping the categories on every edge merely relabels equal-prior gamma categories
        e = int(np.argmax([np.abs(P[0, i] - P[1, i]).max() for i in range(E)]))
        Ps = P.copy()
        Ps[[0, 1], e] = P[[1, 0], e]
        bugs["categories swapped on one edge"] = (m, dict(w, P=Ps))
        bugs["category 0 everywhere"] = (m, dict(w, P=np.ascontiguousarray(np.broadcast_to(P[:1], P.shape))))
    return bugs


@pytest.mark.parametrize("k", sorted(FAMILY_MODELS))
def test_model_detects_plausible_kernel_bugs(oracle, k):
    wl = family_workload(k)
    codes = wl.simulate(48)
    m, w = oracle_model(oracle, wl, codes)
    P = w["P"]
    # the model itself: non-reversible, non-uniform stationary distribution, several rate categories
    assert w["C"] > 1
    assert np.max(np.abs(P - P.transpose(0, 1, 3, 2))) > 1e-3
    assert np.max(w["pi"]) / np.min(w["pi"]) > 1.5
    base = _ll(oracle, m, w, codes, wl.defs)
    assert np.all(np.isfinite(base))
    bugs = _bugs(wl, m, w)
    assert len(bugs) == 4
    for name, (mb, wb) in bugs.items():
        moved = _moved(_ll(oracle, mb, wb, codes, wl.defs), base)
        assert moved > TEETH, (k, name, moved)


def _swap_cherry(codes, b, c):
    out = codes.copy()
    out[[b, c]] = codes[[c, b]]
    return out


@pytest.mark.parametrize("name", K4_MODELS)
def test_k4_model_detects_plausible_kernel_bugs(oracle, name):
    """the k = 4 models: the bugs above where the model has several categories, and
    - the category priors permuted (every model with C > 1 has unequal priors),
    - the two leaf codes of a data-free cherry swapped, on a cherry whose two edge rates differ, at sites where the
      two codes differ (irregular and balanced32: the models whose cherries go through pair tables)"""
    wl = k4_workload(name)
    codes = wl.simulate(48)
    m, w = oracle_model(oracle, wl, codes)
    P, C = w["P"], w["C"]
    assert C == {"irregular": 4, "balanced32": 1, "balanced64": 5, "wide": 2}[name]
    assert np.max(np.abs(P - P.transpose(0, 1, 3, 2))) > 1e-3
    assert np.max(w["pi"]) / np.min(w["pi"]) > 1.5
    base = _ll(oracle, m, w, codes, wl.defs)
    assert np.all(np.isfinite(base))
    bugs = {n: _ll(oracle, mb, wb, codes, wl.defs) for n, (mb, wb) in _bugs(wl, m, w).items()}
    if C > 1:
        prior = w["cat_prior"]
        assert np.max(np.abs(prior - np.roll(prior, 1))) > 0.05
        bugs["category priors permuted"] = _ll(oracle, m, dict(w, cat_prior=np.roll(prior, 1)), codes, wl.defs)
    if name in ("irregular", "balanced32"):
        b, c = cherry_with_unequal_edges(wl, 5.0 if name == "irregular" else 2.0)
        if name == "irregular":
            assert (b, c) == IRREGULAR_CHERRY
        differ = codes[b] != codes[c]
        assert np.sum(differ) >= 5                                   # sites where the orientation of the table shows
        swapped = _ll(oracle, m, w, _swap_cherry(codes, b, c), wl.defs)
        assert np.array_equal(swapped[~differ], base[~differ])
        bugs["cherry codes swapped"] = swapped
    assert len(bugs) == {"irregular": 6, "balanced32": 3, "balanced64": 5, "wide": 5}[name]
    for bug, ll in bugs.items():
        moved = _moved(ll, base)
        assert moved > TEETH, (name, bug, moved)


def test_irregular_model_has_the_shapes_its_name_claims():
    """root with three children, one unary node, one three-way node below the root, two cherry parents (one with data),
    another internal node with data, an edge of rate 0, a rate-0 category, unequal category priors"""
    wl = k4_workload("irregular")
    deg = np.diff(wl.indptr)
    root = int(wl.preorder[0])
    assert wl.T == 13 and deg[root] == 3
    assert np.sum(deg == 1) == 1 and np.sum(deg == 3) == 2 and np.max(deg) == 3
    leaf = deg == 0
    cherries = [a for a in range(wl.N) if deg[a] == 2 and all(leaf[wl.indices[wl.indptr[a]:wl.indptr[a + 1]]])]
    assert len(cherries) == 2 and sum(a in wl.data_nodes for a in cherries) == 1
    assert len(wl.data_nodes) == 2 and np.sum(wl.edge_rates_csr == 0.0) == 1
    k0 = wl.prepare()
    assert k0["cat_rates"][0] == 0.0 and np.allclose(k0["cat_prior"], [0.15, 0.4, 0.05, 0.4], rtol=0, atol=1e-15)
    assert wl.nchar == 7 and k4_workload("wide").nchar == 17


@pytest.mark.parametrize("cfg", [4, 5])
def test_baseline_models_were_blind(cfg):
    """BASELINE configs 4 (k = 20) and 5 (k = 61): symmetric Q, hence uniform pi and symmetric P, and one rate category;
    a transposed P or uniform root weights give the same answer on them"""
    from scipy.linalg import expm

    from phyly_amd import synth
    wl = synth.Workload(cfg)
    Q = np.array(wl.Q)
    k = wl.k
    assert wl.mixture is None                            # C = 1
    assert np.array_equal(Q, Q.T)
    Qd = Q - np.diag(Q.sum(axis=1))
    assert np.max(np.abs(np.full(k, 1.0 / k) @ Qd)) <= 1e-15        # uniform pi is stationary
    P = expm(Qd * wl.edge_rates[0])
    assert np.max(np.abs(P - P.T)) <= 1e-14


def test_gtr_g4_was_blind(oracle):
    """what the engine-level k = 4 tests on synth.Workload gtr_g4 (BASELINE config 3) could not see: its four gamma
    categories have equal priors, so permuting them changes nothing; its root prior is the equilibrium one, the only root
    mode it reaches; its Q is reversible; none of its categories has rate 0; no internal node carries data and every
    internal node has two children.  The other bugs it does see, which is pinned too."""
    from phyly_amd import synth
    wl = synth.Workload(T=24, k=4, tree="yule", model="gtr_g4", seed=3)
    codes = wl.simulate(48)
    m, w = oracle_model(oracle, wl, codes)
    base = _ll(oracle, m, w, codes, wl.defs)
    prior = w["cat_prior"]
    assert np.all(prior == prior[0])
    assert np.array_equal(_ll(oracle, m, dict(w, cat_prior=np.roll(prior, 1)), codes, wl.defs), base)
    assert m.root_mode == 4 and np.array_equal(w["root_w"], w["pi"])              # equilibrium
    pi, Qn = w["pi"], w["Qn"]
    assert np.max(np.abs(pi[:, None] * Qn - (pi[:, None] * Qn).T)) <= 1e-15        # detailed balance: reversible
    assert np.min(w["cat_rates"]) > 0.0
    assert np.all(codes[wl.T:] == wl.k) and set(np.diff(wl.indptr)) == {0, 2}
    wl.root = "equilibrium"
    for bug, (mb, wb) in _bugs(wl, m, w).items():
        assert _moved(_ll(oracle, mb, wb, codes, wl.defs), base) > TEETH, bug
