"""GPU: three-leaf tables in the streamed k = 4 kernel (PLK_OPT_PAIR_TABLES + 1024: a node that is not the root and whose
children are a cherry and a leaf is, with the edge above it, one look-up of a table of nchar^3 rows; the categories may run
in groups, phases of the one launch, to make room) against the same kernel without them (+ 2048) and against the folded
stream without pair products (+ 512).

A row of a three-leaf table is the handlers' own fp64 sequence on the handlers' own operands, and a site's category terms are
added in the same order whatever the groups, so site_ll is compared on its uint64 view with both, and {hi, lo} of the sum bit
for bit with + 2048 (the same waves walk the same units).  All three against the oracle (binary128) at 1e-12.

Shapes, the smallest that can go wrong: the 4-leaf caterpillar (one absorbed node) and the 3-leaf tree (none: the node is
the root, PLK_INFO_LL_TRIPLE says 0); 5-leaf trees in which the absorbed product was followed by a PUSH, a POPMUL, a TIP_MUL
and a plain MATVEC; nchar 4, 5, 6 (and 16, where the combined code is no byte and nothing is absorbed) with C 1, 3, 4, the
categories forced into 1, 2 and C groups (C = 3 in 2 groups: uneven) and S 1, 129, 300; the site count at which some waves
walk two units; site weights; the sum without site_ll; a site of likelihood zero and a rate-0 category; the 40-leaf
caterpillar the program rescales; BASELINE config 3 at S = 300 (absorbed nodes read from the info and set against the byte
budget); the option toggled on a live engine against fresh ones.  The default at these small site counts does not take the
form.  Which nodes qualify, the replay checks and the rows are pinned on the CPU (tests/triplecheck_main.cpp).
"""
import numpy as np
import pytest

from helpers import rel_err, tree_workload
from test_gpu_k4_stream import _codes, _weights, _workload, caterpillar
from test_gpu_k4_fold import _oracle_ll, _shape_edges

pytestmark = pytest.mark.gpu

TOL = 1e-12
DEFAULT, TRIPLE, PLAIN, FOLDED = 1, 1 + 1024, 1 + 2048, 1 + 512
ONE_GROUP, TWO_GROUPS, GROUP_PER_CATEGORY = 4096, 4096 + 8192, 8192
FUSED = 1


@pytest.fixture(scope="module")
def eng():
    from phyly_amd import engine as E
    e = E.Engine(0)
    yield e
    e.set_option(E.OPT_PAIR_TABLES, 1)
    e.close()


def _run(eng, option, per_site=True):
    from phyly_amd import engine as E
    eng.set_option(E.OPT_PAIR_TABLES, option)
    site, (hi, lo) = eng.ll(per_site=per_site)
    what = (eng.info(E.INFO_LL_KERNEL), eng.info(E.INFO_LL_VARIANT), eng.info(E.INFO_LL_FORM), eng.info(E.INFO_LL_PAIRMUL),
            eng.info(E.INFO_LL_TRIPLE))
    return (site.copy() if per_site else None), float(hi), float(lo), what


def _triple_info(v):
    return dict(ran=bool(v & 1), groups=(v >> 4) & 15, nodes=(v >> 8) & 0xFFFF)


def _hl(r):
    return np.array([r[1], r[2]]).view(np.uint64).tolist()


def _three(eng, tag, want, groups=0, ran=True):
    """+ 1024 (+ groups), + 2048, + 512 and the default: the comparisons of the module docstring -> PLK_INFO_LL_TRIPLE as a dict"""
    t = _run(eng, TRIPLE + groups)
    p = _run(eng, PLAIN)
    f = _run(eng, FOLDED)
    d = _run(eng, DEFAULT)
    for r in (t, p, f, d):
        assert r[3][:3] == (FUSED, 6, 1), (tag, r[3])
    info = _triple_info(t[3][4])
    assert p[3][4] == 0 and f[3][4] == 0 and d[3][4] == 0, (tag, p[3], f[3], d[3])
    assert info["ran"] == ran and (ran or t[3][4] == 0), (tag, t[3])
    assert np.all(np.isfinite(p[0]) | np.isneginf(p[0])), tag
    assert np.array_equal(t[0].view(np.uint64), p[0].view(np.uint64)), tag
    assert np.array_equal(t[0].view(np.uint64), f[0].view(np.uint64)), tag
    assert _hl(t) == _hl(p) == _hl(d), (tag, t[1:3], p[1:3])
    if want is not None:
        for name, r in (("three-leaf tables", t), ("without", p), ("folded", f)):
            err = rel_err(r[0], want)
            assert err <= TOL, (tag, name, err)
    print("%s: sum %.17g, %s" % (tag, t[1] + t[2], info))
    return info


def _case(eng, oracle, wl, S, tag, seed=3, groups=0, ran=True):
    wl.setup_engine(eng)
    codes = _codes(wl, S, seed=seed)
    eng.set_patterns_codes(codes, wl.defs)
    eng.set_site_weights(None)
    return _three(eng, "%s S=%d" % (tag, S), _oracle_ll(oracle, wl, codes), groups, ran)


def test_smallest_trees(eng, oracle):
    """(((0, 0), 0), 0): the node above the cherry and its sibling leaf is a look-up; ((0, 0), 0): that node is the root"""
    for S in (1, 129):
        info = _case(eng, oracle, _workload(_shape_edges((((0, 0), 0), 0)), seed=3), S, "four leaves")
        assert info == dict(ran=True, groups=1, nodes=1)
        _case(eng, oracle, _workload(_shape_edges(((0, 0), 0)), seed=4), S, "three leaves", ran=False)


FOLLOWERS = {
    "TIP_MUL": ((((0, 0), 0), 0), 0),                # the parent's next child is a leaf
    "MATVEC": (((((0, 0), 0),), 0), 0),              # a unary node above: the next op is the product of its edge
    "PUSH": (((0, 0), 0), (0, 0)),                   # first of two internal children
    "POPMUL": ((0, 0), ((0, 0), 0)),                 # second of two internal children
}


@pytest.mark.parametrize("follower", list(FOLLOWERS))
def test_what_follows_the_absorbed_product(eng, oracle, follower):
    for groups in (ONE_GROUP, TWO_GROUPS):
        info = _case(eng, oracle, _workload(_shape_edges(FOLLOWERS[follower]), seed=11), 129, follower, groups=groups)
        assert info["nodes"] == 1 and info["groups"] == (1 if groups == ONE_GROUP else 2)


@pytest.mark.parametrize("nchar", [4, 5, 6, 16])
@pytest.mark.parametrize("C", [1, 3, 4])
def test_site_counts_and_groups(eng, oracle, nchar, C):
    """one partly filled unit, two units, a third unit whose second site half is partly filled; 1, 2 and C groups"""
    wl = _workload(caterpillar(8), C=C, nchar=nchar, seed=60 + nchar + C)
    for S in (1, 129, 300):
        for groups, ngroups in ((ONE_GROUP, 1), (TWO_GROUPS, min(2, C)), (GROUP_PER_CATEGORY, C)):
            info = _case(eng, oracle, wl, S, "nchar%d C%d groups%d" % (nchar, C, ngroups), seed=nchar, groups=groups, ran=nchar != 16)
            if nchar != 16:
                assert info == dict(ran=True, groups=ngroups, nodes=1)


def test_two_units_per_wave(eng, oracle):
    """the site count of tests/test_gpu_k4_fold.py: on a GPU of up to 304 CUs some waves walk two units in every phase and the
    others one.  The alignment repeats the columns of a small one, so the oracle is asked for those only."""
    wl = _workload(caterpillar(8), seed=77)
    wl.setup_engine(eng)
    S0 = 128 * 12 * 2 + 5
    block = _codes(wl, S0, seed=9)
    want = _oracle_ll(oracle, wl, block)
    S = 304 * 12 * 128 + S0
    codes = np.ascontiguousarray(np.tile(block, (1, (S + S0 - 1) // S0))[:, :S])
    eng.set_patterns_codes(codes, wl.defs)
    eng.set_site_weights(None)
    info = _three(eng, "units S=%d" % S, np.tile(want, (S + S0 - 1) // S0)[:S], groups=TWO_GROUPS)
    assert info == dict(ran=True, groups=2, nodes=1)


def test_weights_and_sum_only(eng, oracle):
    """site weights with zeros; the sum without site_ll (what an asynchronous evaluation of the sum runs): {hi, lo} bit for bit"""
    wl = _workload(caterpillar(8), seed=21)
    wl.setup_engine(eng)
    codes = _codes(wl, 300, seed=5)
    eng.set_patterns_codes(codes, wl.defs)
    eng.set_site_weights(_weights(300))
    try:
        want = _oracle_ll(oracle, wl, codes)
        for groups in (ONE_GROUP, TWO_GROUPS):
            _three(eng, "weights", want, groups=groups)
            t, p = _run(eng, TRIPLE + groups, per_site=False), _run(eng, PLAIN, per_site=False)
            assert t[3][4] & 1 and p[3][4] == 0 and _hl(t) == _hl(p) == _hl(_run(eng, PLAIN)), (t, p)
    finally:
        eng.set_site_weights(None)


def test_zero_likelihood_site_and_rate0_category(eng, oracle):
    """the irregular tree's mixture (rates 0, 0.4, 1.1, 2.7, unequal priors) on an 8-leaf caterpillar whose cherry has rate 0 on
    both edges: where its leaves disagree the likelihood is exactly 0 (-inf, in every phase no term yet), elsewhere the rate-0
    category contributes through P = I"""
    edges = caterpillar(8)
    rates = [0.0 if child in (0, 1) else 0.1 + 0.03 * i for i, (_, child) in enumerate(edges)]
    wl = tree_workload(4, edges, rates, root="custom", seed=4411, nchar=5, rate_mixture=dict(rates=[0.0, 0.4, 1.1, 2.7], prior=[0.15, 0.4, 0.05, 0.4]))
    wl.setup_engine(eng)
    codes = _codes(wl, 129, seed=8)
    codes[0] = np.minimum(codes[0], 3)
    codes[1] = codes[0]
    codes[0, 2], codes[1, 2] = 0, 1
    eng.set_patterns_codes(codes, wl.defs)
    eng.set_site_weights(None)
    want = _oracle_ll(oracle, wl, codes)
    for groups in (ONE_GROUP, TWO_GROUPS, GROUP_PER_CATEGORY):
        t, p = _run(eng, TRIPLE + groups), _run(eng, PLAIN)
        assert _triple_info(t[3][4])["nodes"] == 1 and np.isneginf(p[0][2]) and np.sum(np.isneginf(p[0])) == 1
        assert np.array_equal(t[0].view(np.uint64), p[0].view(np.uint64)), groups
        keep = np.isfinite(p[0])
        assert rel_err(t[0][keep], want[keep]) <= TOL


def test_rescaled_caterpillar(eng, oracle):
    """40 leaves: SCALE ops stay where they were"""
    for groups in (ONE_GROUP, TWO_GROUPS):
        info = _case(eng, oracle, _workload(caterpillar(40), seed=40), 129, "caterpillar40", groups=groups)
        assert info["nodes"] == 1


def test_config3(eng, oracle):
    """the tables of 4 categories leave room for 2 three-leaf tables, those of 2 for 15, of one for all 16 nodes that qualify:
    (156 KB / categories resident - 200 units x 160 B) / (19 units x 160 B)"""
    from phyly_amd import synth
    wl = synth.Workload(3)
    wl.setup_engine(eng)
    codes = wl.simulate(300)
    eng.set_patterns_codes(codes, wl.defs)
    eng.set_site_weights(None)
    want = _oracle_ll(oracle, wl, codes)
    for groups, ngroups, resident in ((ONE_GROUP, 1, 4), (TWO_GROUPS, 2, 2), (GROUP_PER_CATEGORY, 4, 1)):
        info = _three(eng, "config 3 S=300", want, groups=groups)
        room = 156 * 1024 // resident - 200 * 160                  # the kernel has no static LDS
        assert info["groups"] == ngroups and info["nodes"] == min(16, room // (19 * 160)), info


def test_stale_plan_triple_bits():
    """+ 1024, + 2048 and the group bits toggled on a live engine: after each toggle it answers bit for bit as an engine
    created with that option and reports the same kernel, variant, form, pair products and three-leaf tables"""
    from phyly_amd import engine as E
    wl = _workload(caterpillar(12), seed=41)
    codes = _codes(wl, 300, seed=3)

    def setup(e):
        wl.setup_engine(e)
        e.set_patterns_codes(codes, wl.defs)

    def fresh(option):
        e = E.Engine(0)
        try:
            setup(e)
            return _run(e, option)
        finally:
            e.close()

    live = E.Engine(0)
    try:
        setup(live)
        seen = set()
        for option in (1, TRIPLE, 1, TRIPLE + TWO_GROUPS, PLAIN, TRIPLE + GROUP_PER_CATEGORY, TRIPLE + 512, 6, TRIPLE + ONE_GROUP, 1):
            got, want = _run(live, option), fresh(option)
            assert got[3] == want[3], (option, got[3], want[3])
            assert np.array_equal(got[0].view(np.uint64), want[0].view(np.uint64)) and got[1:3] == want[1:3], option
            seen.add((got[3][2], got[3][4] & 1, (got[3][4] >> 4) & 15))
        # the default and the tile kernel without; one group (also without pair products, which the groups need), two, four
        assert seen == {(1, 0, 0), (0, 0, 0), (1, 1, 1), (1, 1, 2), (1, 1, 4)}, seen
    finally:
        live.close()
