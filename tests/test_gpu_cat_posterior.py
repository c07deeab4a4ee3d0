"""Rate-category posteriors and posterior mean site rates on the GPU: plk_cat_posterior against the oracle helper of
tests/catpost_cases.py, the two kernels against each other, and arbplf-cat-posterior / arbplf-site-rate end to end.

Bound (derived in the issue, catpost_cases.rtol): |post - ref| <= rtol * ref + 1e-300 with
rtol = 4 (E (k + 8) + C + 8) 2^-53, the same for rate; rows of post sum to 1 within (C + 2) 2^-52."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

from helpers import GOLDEN, family_workload, load_json
from phyly_amd import engine as E_, synth
from phyly_amd.engine import Engine, load_library
import catpost_cases as cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "phyly_amd", "csrc")


@pytest.fixture()
def eng():
    e = Engine(0)
    yield e
    e.close()


_compare, _check_engine = cases.compare, cases.check_engine


@pytest.mark.parametrize("name", sorted(cases.SMALL))
def test_engine_matches_oracle_small(eng, oracle, name):
    wl = cases.small_workload(name)
    wl.setup_engine(eng)
    assert wl.prepare()["C"] == cases.SMALL[name][1]
    codes = np.ascontiguousarray(wl.simulate(200))
    eng.set_patterns_codes(codes, wl.defs)
    gp, gr, post, rate = _check_engine(eng, oracle, wl, codes, name, 1)
    cr = wl.prepare()["cat_rates"]
    assert np.max(np.abs(gp @ cr - gr)) <= (len(cr) + 2) * 2.0 ** -52 * np.max(cr)
    if name == "hky85":
        assert np.all(gp == 1) and np.all(gr == 1)
    # the generic kernel on the same inputs: reports 2, agrees with the k = 4 kernel within the bound
    eng.set_option(E_.OPT_FORCE_GENERIC, 1)
    gp2, gr2, _, _ = eng.cat_posterior(want_sums=False)
    assert eng.info(E_.INFO_CAT_POSTERIOR_KERNEL) == 2
    tol = cases.rtol(wl.E, wl.k, len(cr))
    assert np.all(np.abs(gp2 - gp) <= tol * gp + 1e-300) and np.all(np.abs(gr2 - gr) <= tol * gr)
    _compare(name + " generic", gp2, gr2, post, rate, tol)
    eng.set_option(E_.OPT_FORCE_GENERIC, 0)
    # dense patterns (k = 4) take the generic kernel too
    eng.set_patterns_dense(np.ascontiguousarray(wl.defs[codes.T].transpose(1, 2, 0)))
    gp3, gr3, _, _ = eng.cat_posterior(want_sums=False)
    assert eng.info(E_.INFO_CAT_POSTERIOR_KERNEL) == 2
    _compare(name + " dense", gp3, gr3, post, rate, tol)


def test_engine_matches_oracle_100_taxa(eng, oracle):
    """BASELINE config 3 shape, 20 000 sites: the oracle in long double (precise = 1), whose 64-bit mantissa costs the
    same operation count once more at 2^-64: rtol(E, k, C) * 2^-11 is added to the bound"""
    wl = synth.Workload(3)
    wl.setup_engine(eng)
    codes = np.ascontiguousarray(wl.simulate(20000))
    eng.set_patterns_codes(codes, wl.defs)
    extra = cases.rtol(wl.E, wl.k, 4) * 2.0 ** -11
    _check_engine(eng, oracle, wl, codes, "cfg3 20000", 1, precise=1, extra_tol=extra)


def test_nine_categories_and_large_state_spaces_take_the_generic_kernel(eng, oracle):
    wl = cases.MixtureWorkload(T=10, model="gtr_g4", tree="yule", seed=81, mixture=dict(gamma_shape=0.9, gamma_categories=9))
    wl.setup_engine(eng)
    codes = np.ascontiguousarray(wl.simulate(150))
    eng.set_patterns_codes(codes, wl.defs)
    _check_engine(eng, oracle, wl, codes, "C=9", 2)
    for k in (20, 61):
        wl = family_workload(k)
        wl.setup_engine(eng)
        codes = np.ascontiguousarray(wl.simulate(96))
        eng.set_patterns_codes(codes, wl.defs)
        _check_engine(eng, oracle, wl, codes, "k=%d" % k, 2)


def test_rescaling_600_taxa(eng, oracle):
    """site likelihoods ~ e^-830 (tests/test_gpu_hess.py's tree): every category's term lives on its exponent"""
    wl = synth.Workload(T=600, k=4, tree="yule", model="gtr_g4", seed=17)
    wl.setup_engine(eng)
    codes = wl.random_codes(48, seed=4, missing_frac=0.02)
    eng.set_patterns_codes(codes, wl.defs)
    m, w, post, rate, sll = cases.oracle_for(oracle, wl, codes)
    assert np.max(sll) < -700
    gp, gr, _, _, gll, _ = eng.cat_posterior(want_ll=True)
    assert np.all(np.isfinite(gp)) and np.all(np.isfinite(gr))
    _compare("600 taxa", gp, gr, post, rate, cases.rtol(wl.E, wl.k, 4))


def test_does_not_disturb_ll(eng):
    wl = synth.Workload(3)
    wl.setup_engine(eng)
    codes = np.ascontiguousarray(wl.simulate(5000))
    eng.set_patterns_codes(codes, wl.defs)
    a, sa = eng.ll()
    va = eng.info(E_.INFO_LL_VARIANT)
    assert va == 6
    gp, gr, _, _, gll, _ = eng.cat_posterior(want_ll=True)
    assert eng.info(E_.INFO_CAT_POSTERIOR_KERNEL) == 1
    b, sb = eng.ll()
    assert np.array_equal(a, b) and sa == sb and eng.info(E_.INFO_LL_VARIANT) == va
    assert np.max(np.abs(gll - a) / np.abs(a)) <= 1e-15
    # new edge rates between the calls: the posterior call computes P itself, plk_ll still gives what it gives alone
    r2 = wl.edge_rates_csr * 1.1
    eng.update_edge_rates(r2)
    eng.cat_posterior(want_sums=False)
    c, _ = eng.ll()
    eng.update_edge_rates(r2)
    d, _ = eng.ll()
    assert np.array_equal(c, d) and eng.info(E_.INFO_LL_VARIANT) == va


def test_group_equals_single_engine():
    lib = load_library()
    vp, ci, cl = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    lib.plk_group_create.argtypes = [ctypes.POINTER(vp), ci, vp]
    lib.plk_group_destroy.argtypes = [vp]
    lib.plk_group_destroy.restype = None
    lib.plk_group_last_error.argtypes = [vp]
    lib.plk_group_last_error.restype = ctypes.c_char_p
    lib.plk_group_set_tree.argtypes = [vp, ci, vp, vp, vp]
    lib.plk_group_set_model.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp, ci, vp]
    lib.plk_group_set_patterns_codes.argtypes = [vp, cl, vp, ci, vp]
    lib.plk_group_set_site_weights.argtypes = [vp, vp]
    lib.plk_group_cat_posterior.argtypes = [vp, vp, vp, vp, vp]
    wl = cases.small_workload("gtr_g4_i")
    k0 = wl.prepare()
    C, S = k0["C"], 1001
    codes = np.ascontiguousarray(wl.simulate(S))
    w = np.linspace(0.5, 1.5, S)
    P = lambda a: a.ctypes.data_as(vp)
    res = {}
    for G in (1, 2):
        g = vp()
        assert lib.plk_group_create(ctypes.byref(g), G, (ci * G)(*([0] * G))) == 0
        ip, ix, pre = (np.ascontiguousarray(a, dtype=np.int32) for a in (wl.indptr, wl.indices, wl.preorder))
        assert lib.plk_group_set_tree(g, wl.N, P(ip), P(ix), P(pre)) == 0
        Qn, Ql, er = (np.ascontiguousarray(a, dtype=np.float64) for a in (k0["Qn"], k0["Qn_lo"], wl.edge_rates_csr))
        cr, cp, pi = (np.ascontiguousarray(a, dtype=np.float64) for a in (k0["cat_rates"], k0["cat_prior"], k0["pi"]))
        assert lib.plk_group_set_model(g, wl.k, C, P(Qn), P(Ql), P(er), P(cr), P(cp), 4, P(pi)) == 0
        defs = np.ascontiguousarray(wl.defs, dtype=np.float64)
        assert lib.plk_group_set_patterns_codes(g, S, P(codes), wl.nchar, P(defs)) == 0, lib.plk_group_last_error(g)
        assert lib.plk_group_set_site_weights(g, P(w)) == 0
        post, rate, ps, rs = np.zeros((S, C)), np.zeros(S), np.zeros((C, 2)), np.zeros(2)
        assert lib.plk_group_cat_posterior(g, P(post), P(rate), P(ps), P(rs)) == 0, lib.plk_group_last_error(g)
        res[G] = (post, rate, ps.sum(axis=1), rs.sum())
        lib.plk_group_destroy(g)
    assert np.array_equal(res[1][0], res[2][0]) and np.array_equal(res[1][1], res[2][1])
    assert np.max(np.abs(res[1][2] - res[2][2]) / res[1][2]) <= 1e-13
    assert abs(res[1][3] - res[2][3]) <= 1e-13 * res[1][3]


def test_zero_likelihood_site_at_engine_level(eng):
    """site 7 shows two different states at a cherry whose edges have rate 0: likelihood exactly 0"""
    wl = cases.small_workload("gtr_g4")
    k0 = wl.prepare()
    leaf = np.flatnonzero(wl.indptr[1:] == wl.indptr[:-1])
    parent = {int(wl.indices[j]): a for a in range(wl.N) for j in range(wl.indptr[a], wl.indptr[a + 1])}
    pair = next((a, b) for a in leaf for b in leaf if a < b and parent[int(a)] == parent[int(b)])
    rates = wl.edge_rates_csr.copy()
    for j in range(wl.E):
        if int(wl.indices[j]) in pair:
            rates[j] = 0.0
    eng.set_tree(wl.indptr, wl.indices, wl.preorder)
    eng.set_model(k0["Qn"], rates, k0["cat_rates"], k0["cat_prior"], E_.ROOT_EQUILIBRIUM, k0["pi"], Qn_lo=k0["Qn_lo"])
    codes = np.ascontiguousarray(wl.simulate(300))
    codes[pair[0], :] = codes[pair[1], :]
    good = codes.copy()
    codes[pair[0], 7] = (codes[pair[1], 7] + 1) % 4
    for force in (0, 1):
        eng.set_option(E_.OPT_FORCE_GENERIC, force)
        eng.set_patterns_codes(good, wl.defs)
        rp, rr, _, _, rl, _ = eng.cat_posterior(want_ll=True)
        eng.set_patterns_codes(codes, wl.defs)
        gp, gr, _, _, gl, _ = eng.cat_posterior(want_sums=False, want_ll=True)
        assert eng.info(E_.INFO_CAT_POSTERIOR_KERNEL) == 1 + force
        assert np.all(np.isnan(gp[7])) and np.isnan(gr[7]) and gl[7] == -np.inf
        keep = np.arange(300) != 7
        assert np.array_equal(gp[keep], rp[keep]) and np.array_equal(gr[keep], rr[keep]) and np.array_equal(gl[keep], rl[keep])
        with pytest.raises(E_.EngineError, match="site likelihood zero"):
            eng.cat_posterior(per_site=False)
        w = np.ones(300)
        w[7] = 0.0
        eng.set_site_weights(w)                          # weight 0: the site does not enter the sums
        _, _, ps, rs = eng.cat_posterior(per_site=False)
        assert np.all(np.isfinite(ps)) and abs(ps.sum() - 299) <= 1e-9


# ---------------------------------------------------------------------------------------------- operator level
def _same_table(got, want, tol):
    assert got["columns"] == want["columns"] and len(got["data"]) == len(want["data"])
    for a, b in zip(got["data"], want["data"]):
        assert a[:-1] == b[:-1]
        assert abs(a[-1] - b[-1]) <= tol * abs(b[-1]) + 1e-300, (a, b)


def _cli(name, doc):
    p = subprocess.run([os.path.join(CSRC, name)], input=json.dumps(doc).encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    return p.returncode, p.stdout, p.stderr


@pytest.mark.parametrize("example", ["BEAST.GTRG", "BEAST.GTRGI", "BEAST.HKY85I", "BEAST.GTR"])
def test_commands_on_golden_models(oracle, example):
    import arbplf
    md = load_json(os.path.join(GOLDEN, "examples", example, "in.json"))["model_and_data"]
    m = oracle.parse_model(md)
    C = int(oracle.prepare(m)["C"])
    assert (C == 1) == (example == "BEAST.GTR")
    tol = cases.rtol(m.E, m.k, C)             # aggregated cells are sums of non-negative entries: the same relative bound
    S = m.S
    some = sorted(set([0, S // 3, S - 1]))
    site_reds = [None, {"selection": some}, {"aggregation": "sum"}, {"selection": some, "aggregation": "avg"},
                 {"selection": some, "aggregation": [0.5, 2.0, 1.25][:len(some)]}]
    cat_reds = [None, {"selection": sorted({C - 1, 0}, reverse=True)}, {"aggregation": "sum"}, {"aggregation": [float(i + 1) for i in range(C)]}]
    for sr in site_reds:
        base = {"model_and_data": md}
        if sr is not None:
            base["site_reduction"] = sr
        got = json.loads(arbplf.arbplf_site_rate(json.dumps(base)))
        _same_table(got, cases.document_table(oracle, base, "site_rate"), tol)
        for cr in cat_reds:
            doc = dict(base)
            if cr is not None:
                doc["category_reduction"] = cr
            s = arbplf.arbplf_cat_posterior(json.dumps(doc))
            _same_table(json.loads(s), cases.document_table(oracle, doc, "cat_posterior"), tol)
    # algebra: all categories summed give 1 per site; weights equal to the category rates reproduce arbplf-site-rate
    one = json.loads(arbplf.arbplf_cat_posterior(json.dumps({"model_and_data": md, "category_reduction": {"aggregation": "sum"}})))
    assert one["columns"] == ["site", "value"] and all(abs(r[1] - 1) <= (C + 2) * 2.0 ** -52 for r in one["data"])
    rates = [float(v) for v in oracle.prepare(m)["cat_rates"]]
    viar = json.loads(arbplf.arbplf_cat_posterior(json.dumps({"model_and_data": md, "category_reduction": {"aggregation": rates}})))
    direct = json.loads(arbplf.arbplf_site_rate(json.dumps({"model_and_data": md})))
    _same_table(viar, direct, (C + 2) * 2.0 ** -52)
    # CLI and Python: the same bytes
    doc = {"model_and_data": md, "site_reduction": {"aggregation": "avg"}}
    for cli, fn in (("arbplf-cat-posterior", arbplf.arbplf_cat_posterior), ("arbplf-site-rate", arbplf.arbplf_site_rate)):
        rc, out, err = _cli(cli, doc)
        assert rc == 0, err
        assert out.decode().rstrip("\n") == fn(json.dumps(doc))


def test_character_data_file_and_device_groups(tmp_path, monkeypatch):
    import arbplf
    rng = np.random.default_rng(12)
    N, k, S = 9, 4, 3000
    edges = [[8, 0], [8, 7], [7, 1], [7, 6], [6, 2], [6, 5], [5, 3], [5, 4]]
    codes = rng.integers(0, k + 1, (S, N)).astype(np.uint8)
    codes[:, 5:] = k
    md = {"edges": edges, "edge_rate_coefficients": [0.1, 0.2, 0.05, 0.3, 0.15, 0.02, 0.25, 0.4],
          "rate_matrix": [[0, 1, 2, 1], [1, 0, 1, 2], [2, 1, 0, 1], [1, 2, 1, 0]],
          "rate_divisor": "equilibrium_exit_rate", "root_prior": "equilibrium_distribution",
          "gamma_rate_mixture": {"gamma_shape": 0.7, "gamma_categories": 3, "invariable_prior": 0.1},
          "character_definitions": np.vstack([np.eye(k), np.ones((1, k))]).tolist()}
    f = tmp_path / "aln.u8"
    f.write_bytes(codes.tobytes())
    for fn, extra in ((arbplf.arbplf_cat_posterior, {"site_reduction": {"aggregation": "sum"}}),
                      (arbplf.arbplf_cat_posterior, {"site_reduction": {"selection": [0, 17, 2999]}}),
                      (arbplf.arbplf_site_rate, {"site_reduction": {"aggregation": "avg"}}),
                      (arbplf.arbplf_site_rate, {})):
        a = dict(extra, model_and_data=dict(md, character_data=codes.tolist()))
        b = dict(extra, model_and_data=dict(md, character_data_file=str(f)))
        one = json.loads(fn(json.dumps(a)))
        assert one == json.loads(fn(json.dumps(b)))
        monkeypatch.setenv("ARBPLF_DEVICES", "0,0,0")
        three = json.loads(fn(json.dumps(a)))
        monkeypatch.delenv("ARBPLF_DEVICES", raising=False)
        _same_table(three, one, 0.0 if "aggregation" not in extra.get("site_reduction", {}) else 1e-13)


def test_infeasible_site_is_rejected():
    md = load_json(os.path.join(GOLDEN, "examples", "BEAST.GTRG", "in.json"))["model_and_data"]
    md = dict(md, edge_rate_coefficients=[0.0] * len(md["edge_rate_coefficients"]))     # differing leaves: likelihood 0
    for cli in ("arbplf-cat-posterior", "arbplf-site-rate"):
        for red in ({}, {"site_reduction": {"aggregation": "sum"}}):
            rc, out, err = _cli(cli, dict(red, model_and_data=md))
            assert rc != 0 and out == b"" and b"likelihood zero" in err, err
