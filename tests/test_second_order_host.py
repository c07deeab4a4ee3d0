"""Host side of arbplf-inv-hess / -newton-delta / -newton-update (no GPU): plk_solve_second_order through ctypes, its
refusal rule, and the parsing the three commands share with arbplf-hess.

Bound of the solve: the function works in binary128 and rounds once, so against a reference whose own relative error is
cond_inf * E * 2^-52 (long double LU with one step of iterative refinement is better than that) it must agree to that
figure in the max norm."""
import ctypes
import json
import os

import numpy as np
import pytest

from helpers import GOLDEN, load_json
from phyly_amd.engine import load_library
import second_order_cases as cases
from second_order_cases import reference_solve as _reference

PLK_E_ARG = 2
HESS = os.path.join(GOLDEN, "examples", "Felsenstein.2004.fig.16.4", "hess")


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def solve(H, g=None, want_inv=True):
    lib = load_library()
    H = np.asarray(H, dtype=np.longdouble)
    E = H.shape[0]
    hi = H.astype(np.float64)
    lo = (H - hi.astype(np.longdouble)).astype(np.float64)
    hess = np.ascontiguousarray(np.stack([hi, lo], axis=-1))
    grad = None
    if g is not None:
        g = np.asarray(g, dtype=np.float64)
        grad = np.ascontiguousarray(np.stack([g, np.zeros_like(g)], axis=-1))
    inv = np.full((E, E), np.nan) if want_inv else None
    delta = np.full(E, np.nan) if g is not None else None
    cond = ctypes.c_double(np.nan)
    rc = lib.plk_solve_second_order(E, _p(hess), _p(grad), _p(inv), _p(delta), ctypes.byref(cond))
    return rc, inv, delta, cond.value


def _sym(rng, E, definite):
    A = rng.standard_normal((E, E))
    Q, _ = np.linalg.qr(A)
    ev = rng.uniform(0.5, 20.0, E)
    if not definite and E > 1:
        ev[::2] *= -1.0
    H = (Q * ev) @ Q.T
    return (H + H.T) / 2


@pytest.mark.parametrize("E", [1, 2, 18, 198])
@pytest.mark.parametrize("definite", [True, False])
def test_solve_matches_extended_precision(E, definite):
    rng = np.random.default_rng(1000 + E + (7 if definite else 0))
    H = _sym(rng, E, definite)
    g = rng.standard_normal(E)
    rc, inv, delta, cond = solve(H, g)
    assert rc == 0
    Xw, dw = _reference(H, g)
    kappa = float(np.max(np.sum(np.abs(H), axis=1)) * np.max(np.sum(np.abs(Xw), axis=1)))
    assert abs(cond - kappa) <= 1e-6 * kappa
    bound = kappa * E * 2.0 ** -52
    err_inv = float(np.max(np.abs(inv - Xw)) / np.max(np.abs(Xw)))
    err_delta = float(np.max(np.abs(delta - dw)) / np.max(np.abs(dw)))
    print("E=%d definite=%s cond=%.3g inv err %.3g delta err %.3g bound %.3g" % (E, definite, kappa, err_inv, err_delta, bound))
    assert err_inv <= bound and err_delta <= bound
    assert np.array_equal(inv, inv.T)


def test_low_words_of_the_hessian_are_used():
    """the entries are hi + lo: (1, -(1 - 2^-30)) is 2^-30, whose inverse is 2^30 exactly"""
    lib = load_library()
    hess = np.array([[[1.0, -(1.0 - 2.0 ** -30)]]])
    inv = np.zeros((1, 1))
    assert lib.plk_solve_second_order(1, _p(hess), None, _p(inv), None, None) == 0
    assert inv[0, 0] == 2.0 ** 30


def test_singular_and_hopeless_input_is_refused():
    rng = np.random.default_rng(5)
    assert solve(np.zeros((4, 4)), np.ones(4))[0] == PLK_E_ARG
    assert solve(np.zeros((1, 1)))[0] == PLK_E_ARG
    v = rng.standard_normal((6, 2))
    assert solve(v @ v.T)[0] == PLK_E_ARG                  # rank 2 of 6
    # diag(1, t): cond_inf = 1 / t; the rule cond * E * 1e-11 >= 1 refuses t <= E * 1e-11, just above it the solve is done
    E = 2
    t_bad, t_ok = E * 1e-11 * 0.99, E * 1e-11 * 1.02
    rc, _, _, cond = solve(np.diag([1.0, t_bad]))
    assert rc == PLK_E_ARG and cond * E * 1e-11 >= 1
    rc, inv, _, cond = solve(np.diag([1.0, t_ok]))
    assert rc == 0 and cond * E * 1e-11 < 1 and abs(inv[1, 1] * t_ok - 1) < 1e-15


@pytest.mark.parametrize("what", ["inv_hess", "newton_delta", "newton_update"])
def test_validate_shares_the_parsing_of_hess(what):
    lib = load_library()
    lib.arbplf_validate_string.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    for d in ("with.full.data", "with.leaf.data", "with.no.data"):
        with open(os.path.join(HESS, d, "in.json"), "rb") as f:
            assert lib.arbplf_validate_string(what.encode(), f.read()) == 0
    x = load_json(os.path.join(HESS, "with.leaf.data", "in.json"))
    for bad in ({k: v for k, v in x.items() if k != "site_reduction"},
                dict(x, site_reduction={"selection": [0]}),
                dict(x, edge_reduction={"aggregation": "sum"})):
        assert lib.arbplf_validate_string(what.encode(), json.dumps(bad).encode()) != 0
    assert lib.arbplf_validate_string(b"newton_refine", json.dumps(x).encode()) == -1


def test_random_cases_are_well_conditioned_per_the_oracle(oracle):
    """the condition of the GPU test of the three commands on random inputs, checked with the oracle alone: of its 20
    seeded documents at most a quarter may have kappa * E * 1e-11 > 1e-6 (there the bar would show nothing)"""
    counted = 0
    for x in cases.random_documents():
        kappa, E, want = cases.expected(oracle, x)
        print("E=%d kappa=%.3g" % (E, kappa))
        counted += bool(cases.counts(kappa, E, want))
    assert counted >= 15, counted
