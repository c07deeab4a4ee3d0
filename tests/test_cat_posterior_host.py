"""Host side of arbplf-cat-posterior / arbplf-site-rate (no GPU): exports, validation, the loud failure without a
device, and the check of the expected-value helper (tests/catpost_cases.py) against the oracle alone."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import GOLDEN, load_json
from phyly_amd.engine import load_library
import catpost_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GTRGI = os.path.join(GOLDEN, "examples", "BEAST.GTRGI", "in.json")      # gamma_rate_mixture with invariable_prior
GTR = os.path.join(GOLDEN, "examples", "BEAST.GTR", "in.json")          # no mixture


def _validate(what, doc):
    lib = load_library()
    lib.arbplf_validate_string.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    return lib.arbplf_validate_string(what.encode(), json.dumps(doc).encode())


def _categories(doc):
    md = doc["model_and_data"]
    spec = md.get("gamma_rate_mixture") or md.get("normalized_median_gamma_rate_mixture")
    if spec is None:
        return 1
    return spec["gamma_categories"] + (1 if spec.get("invariable_prior", 0) else 0)


def test_library_exports_the_new_entry_points():
    lib = load_library()
    for name in ("plk_cat_posterior", "plk_group_cat_posterior", "arbplf_cat_posterior_string", "arbplf_site_rate_string"):
        assert hasattr(lib, name), name


def test_validate_accepts_and_rejects():
    x = {"model_and_data": load_json(GTRGI)["model_and_data"]}
    plain = {"model_and_data": load_json(GTR)["model_and_data"]}
    C = _categories(x)
    assert C >= 2 and _categories(plain) == 1
    for what in ("cat_posterior", "site_rate"):
        assert _validate(what, x) == 0
        assert _validate(what, plain) == 0                                  # a model without a mixture: one category
        assert _validate(what, dict(x, site_reduction={"selection": [0, 1], "aggregation": "sum"})) == 0
        assert _validate(what, dict(x, bogus_reduction={"aggregation": "sum"})) != 0
    assert _validate("cat_posterior", dict(x, category_reduction={"selection": [0, C - 1]})) == 0
    assert _validate("cat_posterior", dict(x, category_reduction={"aggregation": [1.0] * C})) == 0
    assert _validate("cat_posterior", dict(plain, category_reduction={"selection": [0], "aggregation": "avg"})) == 0
    assert _validate("cat_posterior", dict(x, category_reduction={"selection": [C]})) != 0          # out of range
    assert _validate("cat_posterior", dict(plain, category_reduction={"selection": [1]})) != 0
    assert _validate("cat_posterior", dict(x, category_reduction={"aggregation": [1.0] * (C + 1)})) != 0   # wrong length
    assert _validate("site_rate", dict(x, category_reduction={"aggregation": "sum"})) != 0
    assert _validate("cat_post", x) == -1 and _validate("newton_refine", x) == -1


def test_no_gpu_fails_loudly():
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.is_available())"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    if r.stdout.split()[-1:] == ["True"]:
        pytest.skip("a GPU is present")
    import arbplf
    good = open(GTRGI).read()
    for fn, exe in ((arbplf.arbplf_cat_posterior, "arbplf-cat-posterior"), (arbplf.arbplf_site_rate, "arbplf-site-rate")):
        with pytest.raises(RuntimeError):
            fn(good)
        p = subprocess.run([os.path.join(ROOT, "phyly_amd", "csrc", exe)], input=good.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode != 0 and p.stdout == b"" and b"no CPU fallback" in p.stderr


MIXTURES = {
    "gamma4": dict(gamma_rate_mixture=dict(gamma_shape=0.6, gamma_categories=4)),
    "gamma4_i": dict(gamma_rate_mixture=dict(gamma_shape=0.6, gamma_categories=4, invariable_prior=0.25)),
    "custom_zero_prior": dict(rate_mixture=dict(rates=[0.1, 0.7, 1.5, 3.0], prior=[0.3, 0.0, 0.5, 0.2])),
    "none": {},
}


@pytest.mark.parametrize("name", sorted(MIXTURES))
def test_helper_reproduces_the_mixture_log_likelihood(oracle, name):
    """log-sum-exp over categories of log prior_c + log L_{s,c} is the oracle's own site log likelihood of the mixture"""
    md = {k: v for k, v in load_json(GTR)["model_and_data"].items()
          if k not in ("rate_mixture", "gamma_rate_mixture", "normalized_median_gamma_rate_mixture")}
    md.update(MIXTURES[name])
    m = oracle.parse_model(md)
    w = oracle.prepare(m)
    assert int(w["C"]) == {"gamma4": 4, "gamma4_i": 5, "custom_zero_prior": 4, "none": 1}[name]
    post, rate, sll = cases.posteriors(oracle, m, w, B=m.B)
    want, _ = oracle.site_ll(m, w, B=m.B, precise=2)
    err = float(np.max(np.abs(sll - want) / np.abs(want)))
    print("%s: %d sites, helper vs oracle %.3g" % (name, len(want), err))
    assert np.all(np.isfinite(want)) and err <= 1e-15
    assert np.all(np.abs(np.sum(post, axis=1) - 1) <= 2.0 ** -60)
    prior = np.asarray(w["cat_prior"])
    assert np.all(post[:, prior == 0] == 0)
    if name == "none":
        assert np.all(post == 1) and np.all(rate == 1)
