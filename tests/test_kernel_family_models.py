"""CPU only: the models of tests/test_gpu_kernel_families.py can tell a wrong kernel from a right one.

For every state count there, the oracle alone shows that a plausible kernel bug moves the per-site log likelihood by far
more than the 1e-12 tolerance of the GPU tests: P read transposed, uniform root weights (or, for a uniform root prior,
the equilibrium ones: root modes mixed up), the matrices of two rate categories swapped on one edge (a stride mistake),
every category given category 0's matrices.  Also pinned: why the BASELINE models were blind to all of these (symmetric
Q, uniform pi, symmetric P, one rate category)."""
import copy

import numpy as np
import pytest

from helpers import FAMILY_MODELS, family_workload, oracle_model

TEETH = 1e-6        # a bug must move some site's ll by this much (relative to max(1, |ll|)), >> the 1e-12 GPU tolerance


def _ll(oracle, m, w, codes, defs):
    ll, _ = oracle.site_ll(m, w, codes=np.ascontiguousarray(codes.T), defs=defs, precise=1)   # precise=1 reads w["P"]
    return ll


def _moved(a, b):
    return np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))


@pytest.mark.parametrize("k", sorted(FAMILY_MODELS))
def test_model_detects_plausible_kernel_bugs(oracle, k):
    wl = family_workload(k)
    codes = wl.simulate(48)
    m, w = oracle_model(oracle, wl, codes)
    C, E = w["C"], wl.E
    P = w["P"]
    # the model itself: non-reversible, non-uniform stationary distribution, several rate categories
    assert C > 1
    assert np.max(np.abs(P - P.transpose(0, 1, 3, 2))) > 1e-3
    assert np.max(w["pi"]) / np.min(w["pi"]) > 1.5
    base = _ll(oracle, m, w, codes, wl.defs)
    assert np.all(np.isfinite(base))

    bugs = {}
    bugs["P transposed"] = (m, dict(w, P=np.ascontiguousarray(P.transpose(0, 1, 3, 2))))
    mu = copy.copy(m)
    mu.root_mode = 2                                     # custom weights
    if wl.root == "uniform":
        rw = w["pi"].copy()                              # uniform <-> equilibrium mixed up
    else:
        rw = np.full(k, 1.0 / k)
    bugs["root weights"] = (mu, dict(w, root_w=rw))
    # one edge only: swapping the categories on every edge merely relabels equal-prior gamma categories
    e = int(np.argmax([np.abs(P[0, i] - P[1, i]).max() for i in range(E)]))
    Ps = P.copy()
    Ps[[0, 1], e] = P[[1, 0], e]
    bugs["categories swapped on one edge"] = (m, dict(w, P=Ps))
    bugs["category 0 everywhere"] = (m, dict(w, P=np.ascontiguousarray(np.broadcast_to(P[:1], P.shape))))
    for name, (mb, wb) in bugs.items():
        moved = _moved(_ll(oracle, mb, wb, codes, wl.defs), base)
        assert moved > TEETH, (k, name, moved)


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
