"""GPU: the frame of the streamed k = 4 kernel around its interpreter statement -- the per-category record the statement loads
its operands and the root weights from, units counted in 32 bits, a site's state between the categories as sum and exponent
alone (plk_mix_term: "no term yet" is the exponent's sentinel), and in phases after the first the partial sums requested a
unit ahead.

None of it may change a bit: site_ll is compared on its uint64 view across the default, the tile kernel (PLK_OPT_PAIR_TABLES 5),
the stream without tables (+ 2048), the categories forced into 1 / 2 / C groups, and the barrier variants (+ 16, + 32, + 65536)
of the default and of the group-per-category plan; {hi, lo} of the sum bit for bit across the streamed runs of one workgroup
cap (the same waves walk the same units; the tile kernel adds its double-double partial sums in another order, so its sum is
held to 4 ulp of the double).  All of them against the oracle (binary128) at 1e-12.

Shapes: BASELINE config 3's tree at S = 300, and at S = 12 x 128 x 3 + 77 = 4685 under PLK_OPT_STREAM_GRID 1 and 2 (waves with
several units, a partial last pass and the wrap between phases: where a request a unit ahead can go wrong); the 40-leaf
caterpillar, which rescales, so that exponents differ between the categories; C = 1 and C = 4; a rate-0 category, a category of
prior 0 and a site of likelihood zero (-inf) in one mixture; S = 129 and S = 1 (padding lanes); and a root-weight change between
two evaluations on one engine, without a pattern upload, against a fresh engine.
"""
import copy

import numpy as np
import pytest

from helpers import rel_err, tree_workload
from test_gpu_k4_stream import _workload, caterpillar
from test_gpu_k4_fold import _oracle_ll
from test_gpu_k4_quad import _qcodes

pytestmark = pytest.mark.gpu

TOL = 1e-12
DEFAULT, TILE, PLAIN, QUAD = 1, 5, 1 + 2048, 1 + 16384
ONE_GROUP, TWO_GROUPS, GROUP_PER_CATEGORY = 4096, 4096 + 8192, 8192
BARRIERS = (16, 32, 65536)
BIG = 12 * 128 * 3 + 77


@pytest.fixture(scope="module")
def eng():
    from phyly_amd import engine as E
    e = E.Engine(0)
    yield e
    e.set_option(E.OPT_PAIR_TABLES, 1)
    e.set_option(E.OPT_STREAM_GRID, 0)
    e.close()


def _run(eng, option, grid=0):
    from phyly_amd import engine as E
    eng.set_option(E.OPT_STREAM_GRID, grid)
    eng.set_option(E.OPT_PAIR_TABLES, option)
    site, (hi, lo) = eng.ll()
    what = dict(form=eng.info(E.INFO_LL_FORM), groups=(eng.info(E.INFO_LL_TRIPLE) >> 4) & 15, barrier=eng.info(E.INFO_LL_BARRIER) & 3)
    assert eng.info(E.INFO_LL_KERNEL) == 1 and eng.info(E.INFO_LL_VARIANT) == 6, option
    return site.copy(), np.array([float(hi), float(lo)]), what


def _variants(C):
    v = [("default", DEFAULT), ("without tables", PLAIN), ("one group", QUAD + ONE_GROUP), ("two groups", QUAD + TWO_GROUPS),
         ("group per category", QUAD + GROUP_PER_CATEGORY)]
    v += [("default + %d" % b, DEFAULT + b) for b in BARRIERS] + [("group per category + %d" % b, QUAD + GROUP_PER_CATEGORY + b) for b in BARRIERS]
    return v


def _all_forms(eng, tag, want, C, grids=(0,), groups_expected=True):
    """every variant under every workgroup cap: equal bits, the oracle at TOL -> the default's site_ll"""
    tile = _run(eng, TILE)
    assert tile[2]["form"] == 0, (tag, tile[2])
    finite = np.isfinite(want)
    assert np.array_equal(np.isneginf(tile[0]), ~finite), tag
    first = None
    seen = set()
    for grid in grids:
        base = None
        for name, option in _variants(C):
            site, hl, what = _run(eng, option, grid)
            t = "%s, %s, cap %d" % (tag, name, grid)
            assert what["form"] == 1, (t, what)
            assert np.array_equal(site.view(np.uint64), tile[0].view(np.uint64)), t
            if base is None:
                base = hl
                if first is None:
                    first = site
                    err = rel_err(site[finite], want[finite])
                    print("%s: rel err %.3g, sum %.17g" % (t, err, hl.sum()))
                    assert err <= TOL, (t, err)
            if finite.all():
                assert hl.view(np.uint64).tolist() == base.view(np.uint64).tolist(), (t, hl, base)
            seen.add(what["groups"])
        if finite.all():
            assert abs(base.sum() - tile[1].sum()) <= 4 * 2.3e-16 * abs(base.sum()), (tag, grid, base, tile[1])
    if groups_expected:
        assert {1, min(2, C), C} <= seen, (tag, seen)
    return first


def _config3(oracle):
    from phyly_amd import synth
    wl = synth.Workload(3)
    codes = wl.simulate(BIG)
    return wl, codes, _oracle_ll(oracle, wl, codes)


_shared = {}


def _config3_once(oracle):
    if "config3" not in _shared:
        wl, codes, want = _config3(oracle)
        want.setflags(write=False)
        _shared["config3"] = (wl, codes, want)
    return _shared["config3"]


def test_config3_s300(eng, oracle):
    wl, codes, want = _config3_once(oracle)
    wl.setup_engine(eng)
    eng.set_patterns_codes(np.ascontiguousarray(codes[:, :300]), wl.defs)
    eng.set_site_weights(None)
    _all_forms(eng, "config 3 S=300", want[:300], 4)


@pytest.mark.parametrize("grid", [1, 2])
def test_config3_several_units_a_wave(eng, oracle, grid):
    wl, codes, want = _config3_once(oracle)
    wl.setup_engine(eng)
    eng.set_patterns_codes(codes, wl.defs)
    eng.set_site_weights(None)
    got = _all_forms(eng, "config 3 S=%d" % BIG, want, 4, grids=(grid,))
    uncapped = _run(eng, DEFAULT, 0)
    assert np.array_equal(got.view(np.uint64), uncapped[0].view(np.uint64))


@pytest.mark.parametrize("C", [1, 4])
@pytest.mark.parametrize("S", [1, 129])
def test_rescaled_caterpillar(eng, oracle, C, S):
    """40 leaves: the program rescales, the categories' exponents differ, and the last unit is mostly padding"""
    wl = _workload(caterpillar(40), C=C, seed=140 + C)
    wl.setup_engine(eng)
    codes = _qcodes(wl, S, 9)
    eng.set_patterns_codes(codes, wl.defs)
    eng.set_site_weights(None)
    _all_forms(eng, "caterpillar40 C%d S=%d" % (C, S), _oracle_ll(oracle, wl, codes), C)


def test_caterpillar_several_units_a_wave(eng, oracle):
    wl = _workload(caterpillar(40), C=4, seed=144)
    wl.setup_engine(eng)
    codes = _qcodes(wl, BIG, 10)
    eng.set_patterns_codes(codes, wl.defs)
    eng.set_site_weights(None)
    _all_forms(eng, "caterpillar40 S=%d" % BIG, _oracle_ll(oracle, wl, codes), 4, grids=(1, 2))


def test_zero_terms(eng, oracle):
    """a rate-0 category (P = I), a category of prior 0 (its term is zero at every site: first, in the middle or last in its
    phase, whatever the groups) and a site of likelihood zero (every term zero: -inf): an 8-leaf caterpillar whose cherry has
    rate 0 on both edges, so that under every category the likelihood is 0 where its leaves disagree"""
    edges = caterpillar(8)
    rates = [0.0 if child in (0, 1) else 0.1 + 0.03 * i for i, (_, child) in enumerate(edges)]
    for prior in ([0.15, 0.0, 0.45, 0.4], [0.0, 0.3, 0.3, 0.4], [0.2, 0.4, 0.4, 0.0]):
        wl = tree_workload(4, edges, rates, root="custom", seed=4411, nchar=5, rate_mixture=dict(rates=[0.0, 0.4, 1.1, 2.7], prior=prior))
        wl.setup_engine(eng)
        codes = _qcodes(wl, 129, 8)
        codes[1] = codes[0]
        codes[0, 2], codes[1, 2] = 0, 1
        eng.set_patterns_codes(codes, wl.defs)
        eng.set_site_weights(None)
        want = _oracle_ll(oracle, wl, codes)
        assert np.isneginf(want[2]) and np.sum(~np.isfinite(want)) == 1
        got = _all_forms(eng, "zero terms, prior %s" % prior, want, 4)
        assert np.isneginf(got[2]) and np.sum(np.isneginf(got)) == 1


def test_root_weights_follow_the_model(oracle):
    """the root weights sit in the records written with the formats: a model that differs in them alone, set between two
    evaluations without a pattern upload, must answer as a fresh engine does -- custom to custom, to none, to uniform, back"""
    from phyly_amd import engine as E
    wl = _workload(caterpillar(12), root="custom", seed=151)
    codes = _qcodes(wl, 300, 4)
    others = []
    for i, root in enumerate(("custom", "none", "uniform", "custom")):
        w2 = copy.copy(wl)
        w2.root = root
        w2.root_custom = np.random.default_rng(900 + i).uniform(0.05, 1.0, 4) if root == "custom" else None
        others.append(w2)

    def fresh(w, option):
        e = E.Engine(0)
        try:
            w.setup_engine(e)
            e.set_patterns_codes(codes, w.defs)
            return _run(e, option)
        finally:
            e.close()

    live = E.Engine(0)
    try:
        wl.setup_engine(live)
        live.set_patterns_codes(codes, wl.defs)
        previous = _run(live, DEFAULT)[0]
        for w2 in others:
            k0 = w2.prepare()
            mode, rw = w2.root_engine()
            live.set_model(k0["Qn"], w2.edge_rates_csr, k0["cat_rates"], k0["cat_prior"], mode, rw, Qn_lo=k0["Qn_lo"])
            for option in (DEFAULT, QUAD + GROUP_PER_CATEGORY, PLAIN):
                got, want = _run(live, option), fresh(w2, option)
                assert np.array_equal(got[0].view(np.uint64), want[0].view(np.uint64)), (w2.root, option)
                assert got[1].view(np.uint64).tolist() == want[1].view(np.uint64).tolist(), (w2.root, option)
            assert not np.array_equal(got[0], previous), w2.root
            assert rel_err(got[0], _oracle_ll(oracle, w2, codes)) <= TOL, w2.root
            previous = got[0]
    finally:
        live.close()
