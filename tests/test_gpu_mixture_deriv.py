"""GPU: arbplf-mixture-deriv end to end -- the gamma forms against central differences of the oracle's arbplf_ll on the
reference's example data, a custom mixture under the exit-rate divisor against the oracle expectations of
tests/mixsens_cases.py combined by the closed-form chain, "avg" against "sum", and the command against the Python call."""
import copy
import json
import os
import subprocess

import numpy as np
import pytest

import mixsens_cases as cases
import qgrad_cases
from helpers import GOLDEN, load_json

pytestmark = pytest.mark.gpu
LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GTRGI = os.path.join(GOLDEN, "examples", "BEAST.GTRGI", "in.json")
SUM = {"aggregation": "sum"}


def _call(md, red=SUM):
    import arbplf
    out = json.loads(arbplf.arbplf_mixture_deriv(json.dumps({"model_and_data": md, "site_reduction": red})))
    assert out["columns"] == ["parameter", "category", "value"]
    return out["data"]


def _cli(md, red=SUM, env=None):
    p = subprocess.run([os.path.join(ROOT, "phyly_amd", "csrc", "arbplf-mixture-deriv")],
                       input=json.dumps({"model_and_data": md, "site_reduction": red}).encode(),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **(env or {})))
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout)["data"]


def _five_point(f, x, h):
    return (f(x - 2 * h) - 8 * f(x - h) + 8 * f(x + h) - f(x + 2 * h)) / (12 * LD(h))


def gamma_doc(key):
    """the reference's BEAST.GTRGI example: as shipped (normalized median gamma + I) or with the same numbers as a
    gamma_rate_mixture (category means): Gamma4 + I"""
    md = copy.deepcopy(load_json(GTRGI)["model_and_data"])
    spec = md.pop("normalized_median_gamma_rate_mixture")
    md[key] = spec
    return md


@pytest.mark.parametrize("key", ["gamma_rate_mixture", "normalized_median_gamma_rate_mixture"])
def test_gamma_forms_against_central_differences_of_the_oracle(oracle, key):
    """5-point central differences of oracle.arbplf_ll at steps h and h / 2.  The oracle prints a double: rounding
    1.5 ulp(ll) / h, so the bar is the larger of 1e-9 and ten times the disagreement of the two steps, and the
    disagreement itself must stay below 1e-8."""
    md = gamma_doc(key)
    rows = _call(md)
    assert [r[:2] for r in rows] == [["gamma_shape", 0], ["invariable_prior", 0]]

    def ll(param, x):
        d = copy.deepcopy(md)
        d[key][param] = float(x)
        return LD(json.loads(oracle.arbplf_ll(json.dumps({"model_and_data": d, "site_reduction": SUM})))["data"][0][-1])

    for (name, _, got), h in zip(rows, (2e-3, 2e-3)):
        x0 = md[key][name]
        a, b = _five_point(lambda x: ll(name, x), x0, h * x0 / 2), _five_point(lambda x: ll(name, x), x0, h * x0)
        gap = float(abs(a - b) / abs(a))
        err = float(abs(LD(got) - a) / abs(a))
        print("%s d/d%s = %.12g: %.3g relative to the central difference (steps disagree by %.3g)" % (key, name, got, err, gap))
        assert gap < 1e-8
        assert err <= max(1e-9, 10 * gap)
    # no invariable category: one row only
    md0 = copy.deepcopy(md)
    del md0[key]["invariable_prior"]
    assert [r[:2] for r in _call(md0)] == [["gamma_shape", 0]]


def test_custom_mixture_exit_rate_divisor(oracle):
    """rate_mixture with array prior under "equilibrium_exit_rate": the divisor carries expect = sum r p.  Expected:
    (prior_out, rate_out) from the oracle on the same model written with the numeric divisor exit_rate * expect, then the
    closed-form chain.  Bound 1e-11 of max|rate_out| resp. max|prior_out|: the device sums are held to 1e-12 and the
    divisor is rounded to a double once."""
    rates, prior = [0.3, 1.0, 2.2], [0.5, 0.3, 0.2]
    md = cases.five_taxon_doc(70, 4, seed=51, mixture={"rate_mixture": {"rates": rates, "prior": prior}}, divisor="equilibrium_exit_rate")
    wts = [float(v) for v in np.random.default_rng(8).uniform(0.0, 2.0, 70)]
    _, _, d = qgrad_cases.normalised(md["rate_matrix"], "equilibrium_exit_rate")
    expect = sum(LD(r) * LD(p) for r, p in zip(rates, prior))
    po, ro, _ = cases.expectations(oracle, dict(md, rate_divisor=float(d * expect)), wts)
    wr, wp = cases.closed_form_chain(rates, prior, True, po, ro)
    rows = _call(md, {"aggregation": wts})
    assert [r[:2] for r in rows] == [["rate", c] for c in range(3)] + [["prior", c] for c in range(3)]
    got = np.array([r[2] for r in rows], dtype=LD)
    er = float(np.max(np.abs(got[:3] - wr)) / np.max(np.abs(ro)))
    ep = float(np.max(np.abs(got[3:] - wp)) / np.max(np.abs(po)))
    print("custom mixture, exit-rate divisor: d/drates %.3g of max|rate_out|, d/dprior %.3g of max|prior_out| (bound 1e-11)" % (er, ep))
    assert er <= 1e-11 and ep <= 1e-11
    # uniform prior: rates only
    mdu = dict(md, rate_mixture={"rates": rates, "prior": "uniform_distribution"})
    assert [r[:2] for r in _call(mdu)] == [["rate", c] for c in range(3)]


def test_avg_is_sum_over_selected_sites():
    md = gamma_doc("gamma_rate_mixture")
    sel = [0, 3, 3, 10, 40]
    s = _call(md, {"selection": sel, "aggregation": "sum"})
    a = _call(md, {"selection": sel, "aggregation": "avg"})
    for rs, ra in zip(s, a):
        assert rs[:2] == ra[:2] and abs(ra[2] - rs[2] / len(sel)) <= 4e-16 * abs(ra[2])


def test_command_prints_the_table_of_the_python_call():
    md = gamma_doc("normalized_median_gamma_rate_mixture")
    assert _cli(md) == _call(md)
    # dense observations kept dense (generic kernel) give the compact answer
    dense = cases.five_taxon_doc(70, 4, seed=52, dense=True)
    a, b = _cli(dense), _cli(dense, env={"ARBPLF_COMPACT_DENSE": "0"})
    scale = max(abs(r[2]) for r in a)
    assert [r[:2] for r in a] == [r[:2] for r in b] and max(abs(x[2] - y[2]) for x, y in zip(a, b)) <= 1e-12 * scale
    # a model without a mixture is refused with a diagnostic
    plain = {key: v for key, v in md.items() if key not in cases.MIX_KEYS}
    p = subprocess.run([os.path.join(ROOT, "phyly_amd", "csrc", "arbplf-mixture-deriv")],
                       input=json.dumps({"model_and_data": plain, "site_reduction": SUM}).encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode != 0 and b"no rate mixture" in p.stderr
