"""Host side of arbplf-mixture-deriv (no GPU): exports, validation and the chain rule of plk_mixture_chain on hand-made
(prior_out, rate_out): the gamma forms against central differences of the oracle's gamma_mixture, the exit-rate terms of a
custom mixture against the closed form."""
import ctypes
import json
import os
from fractions import Fraction

import numpy as np
import pytest

import mixsens_cases as cases
from helpers import GOLDEN, load_json
from phyly_amd.engine import load_library

LD = np.longdouble
GTRGI = os.path.join(GOLDEN, "examples", "BEAST.GTRGI", "in.json")


def _validate(what, doc):
    lib = load_library()
    lib.arbplf_validate_string.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    return lib.arbplf_validate_string(what.encode(), json.dumps(doc).encode())


def test_library_exports_the_new_entry_points():
    lib = load_library()
    for name in ("plk_mixture_sens", "plk_group_mixture_sens", "plk_mixture_chain", "arbplf_mixture_deriv_string"):
        assert hasattr(lib, name), name
    import arbplf
    assert callable(arbplf.arbplf_mixture_deriv)


def test_validate_accepts_and_rejects():
    md = load_json(GTRGI)["model_and_data"]
    S = len(md["character_data"])
    x = {"model_and_data": md}
    ok = lambda red: _validate("mixture_deriv", dict(x, site_reduction=red))
    assert ok({"aggregation": "sum"}) == 0
    assert ok({"aggregation": "avg"}) == 0
    assert ok({"aggregation": [0.5] * S}) == 0
    assert ok({"selection": [0, 2], "aggregation": [1.5, 2.0]}) == 0
    assert _validate("mixture_deriv", x) != 0                                          # no site_reduction
    assert ok({"selection": [0, 1]}) != 0                                              # not aggregating
    assert _validate("mixture_deriv", dict(x, site_reduction={"aggregation": "sum"}, edge_reduction={"aggregation": "sum"})) != 0
    plain = {key: v for key, v in md.items() if key not in cases.MIX_KEYS}
    assert _validate("mixture_deriv", {"model_and_data": plain, "site_reduction": {"aggregation": "sum"}}) != 0     # no mixture
    custom = dict(plain, rate_mixture={"rates": [0.5, 2.0], "prior": "uniform_distribution"})
    assert _validate("mixture_deriv", {"model_and_data": custom, "site_reduction": {"aggregation": "sum"}}) == 0


def _five_point(f, x, h):
    return (f(x - 2 * h) - 8 * f(x - h) + 8 * f(x + h) - f(x + 2 * h)) / (12 * LD(h))


def _fd(f, x, h):
    """5-point central difference at steps h and h / 2 -> (value at h / 2, their disagreement)"""
    a, b = _five_point(f, x, h / 2), _five_point(f, x, h)
    return a, abs(a - b)


@pytest.mark.parametrize("pinv", [0.0, 0.2])
@pytest.mark.parametrize("shape", [0.3, 1.0, 7.5])
@pytest.mark.parametrize("n", [1, 4, 5])
@pytest.mark.parametrize("mode", ["mean", "median"])
def test_gamma_chain_against_central_differences(oracle, mode, n, shape, pinv):
    """F(shape, pinv) = sum_c prior_out[c] p_c + rate_out[c] r_c is linear in (p, r), so its derivatives are what the chain
    returns.  Bar: the larger of 1e-9 and ten times the disagreement of steps h and h / 2 (itself asserted below 1e-8),
    relative to the size of the terms."""
    omode, pmode = (3, 4) if mode == "mean" else (4, 5)
    C = n + (1 if pinv else 0)
    rng = np.random.default_rng(n * 100 + int(shape * 10) + (7 if pinv else 0))
    po, ro = rng.uniform(-2, 3, C), rng.uniform(-2, 3, C)

    def F(a, q):
        r, p = oracle.gamma_mixture(omode, n, float(a), float(q))
        assert len(r) == C
        return np.sum(np.asarray(po, dtype=LD) * np.asarray(p, dtype=LD) + np.asarray(ro, dtype=LD) * np.asarray(r, dtype=LD))

    got = cases.product_chain(pmode, n, None, None, shape, pinv, False, po, ro)
    assert got["rc"] == 0, got["msg"]
    r0, _ = oracle.gamma_mixture(omode, n, shape, pinv)
    s_shape = float(np.sum(np.abs(ro[:n]) * r0[:n]) / shape)
    want, gap = _fd(lambda a: F(a, pinv), shape, 2e-3 * shape)
    assert gap / s_shape < 1e-8
    err = float(abs(got["dshape"] - want) / s_shape)
    msg = "%s n=%d shape=%g pinv=%g: d/dshape %.3g (bound %.3g)" % (mode, n, shape, pinv, err, max(1e-9, 10 * gap / s_shape))
    assert err <= max(1e-9, 10 * gap / s_shape), msg
    if not pinv:
        assert got["has_inv"] == 0 and np.isnan(got["dinv"])          # no invariable category: nothing reported, nothing written
        print(msg)
        return
    assert got["has_inv"] == 1
    s_inv = float(np.sum(np.abs(ro[:n]) * r0[:n]) / (1 - pinv) + np.sum(np.abs(po)))
    want, gap = _fd(lambda q: F(shape, q), pinv, 2e-3)
    assert gap / s_inv < 1e-8
    err = float(abs(got["dinv"] - want) / s_inv)
    print(msg + "; d/dinvariable_prior %.3g (bound %.3g)" % (err, max(1e-9, 10 * gap / s_inv)))
    assert err <= max(1e-9, 10 * gap / s_inv)


def test_custom_mixture_exit_rate_terms():
    rng = np.random.default_rng(5)
    rates, prior = [0.3, 1.0, 2.2], [0.5, 0.3, 0.2]
    po, ro = rng.uniform(-3, 3, 3), rng.uniform(-3, 3, 3)
    for exit_rate in (False, True):
        got = cases.product_chain(2, 3, rates, prior, 1.0, 0.0, exit_rate, po, ro)
        assert got["rc"] == 0, got["msg"]
        wr, wp = cases.closed_form_chain(rates, prior, exit_rate, po, ro)
        er = float(np.max(np.abs(got["drates"] - wr)) / np.max(np.abs(wr)))
        ep = float(np.max(np.abs(got["dprior"] - wp)) / np.max(np.abs(wp)))
        print("custom mixture, exit rate %s: d/drates %.3g, d/dprior %.3g (bound 2.3e-16: one rounding to double)" % (exit_rate, er, ep))
        assert er <= 2.3e-16 and ep <= 2.3e-16
        if not exit_rate:
            assert np.array_equal(got["drates"], ro) and np.array_equal(got["dprior"], po)
    # uniform prior: rates only, p_c = 1 / n
    got = cases.product_chain(3, 3, rates, None, 1.0, 0.0, True, po, ro)
    assert got["rc"] == 0, got["msg"]
    wr, _ = cases.closed_form_chain(rates, None, True, po, ro)
    assert float(np.max(np.abs(got["drates"] - wr)) / np.max(np.abs(wr))) <= 2.3e-16
    assert np.all(np.isnan(got["dprior"]))                               # not written


def test_exit_rate_invariance_in_binary128():
    """Under the exit-rate divisor scaling every rate changes nothing: sum_c r_c d/drates[c] = 0.  On dyadic inputs (expect
    = 1, every product and quotient exact in binary128 and in double) the rounded outputs must satisfy it to 1e-28 of the
    terms, which any arithmetic narrower than binary128 in the chain would miss on the second input set."""
    for rates, prior, ro in (([0.5, 1.0, 2.0], [0.5, 0.25, 0.25], [3.0, -5.0, 7.0]),
                             ([0.5, 1.0, 2.0], [0.5, 0.25, 0.25], [3.0 + 2.0 ** -40, -5.0, 7.0 - 2.0 ** -42])):
        got = cases.product_chain(2, 3, rates, prior, 1.0, 0.0, True, [1.0, 1.0, 1.0], ro)
        assert got["rc"] == 0, got["msg"]
        terms = [Fraction(r) * Fraction(float(d)) for r, d in zip(rates, got["drates"])]
        total, size = sum(terms), sum(abs(t) for t in terms)
        print("sum r d/drates = %.3g of the terms (bound 1e-28)" % float(abs(total) / size))
        assert abs(total) <= Fraction(1, 10 ** 28) * size


def test_refusals():
    got = cases.product_chain(2, 3, [0.0, 0.0, 0.0], [0.5, 0.3, 0.2], 1.0, 0.0, True, [1, 1, 1], [1, 2, 3])
    assert got["rc"] != 0 and "expected rate" in got["msg"]
    got = cases.product_chain(2, 3, [0.0, 0.0, 0.0], [0.5, 0.3, 0.2], 1.0, 0.0, False, [1, 1, 1], [1, 2, 3])
    assert got["rc"] == 0                                                 # a fixed divisor does not need the expectation
    got = cases.product_chain(1, 1, None, None, 1.0, 0.0, False, [1], [1])
    assert got["rc"] != 0 and "no rate mixture" in got["msg"]
