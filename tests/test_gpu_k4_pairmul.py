"""GPU: the pair-product form of the streamed k = 4 kernel (k_ll_fused4_v4s<768, true, true>, the default PLK_OPT_PAIR_TABLES 1 for trees
within 3 stack slots: a second look-up buffer in the registers of slot 3, the look-up chain two observations ahead, two
table rows multiplied under one dispatch) against the folded stream on k_ll_fused4_v4s (+ 512, the default before it) and
against the 1536-site tile kernel (6, or 5 where 6 does not fit).

The three run the same multiplies on the same operands per site, so site_ll is compared on its uint64 view.  Default and
+ 512 give the same wave the same units in the same order: {hi, lo} of the sum equal bit for bit.  The tile kernel sums in
another order: hi + lo within 1e-13 relative.  All three against the oracle (binary128) at 1e-12.

Shapes, the smallest that can go wrong: a 3-leaf tree (the PAIR is the program's first and last observation op) and a 4-leaf
balanced tree (two pair tables under the root); caterpillars and balanced trees of 3 .. 12 leaves and the same below a root
with one more leaf (both buffer parities, an ADVANCE before and inside a PAIR, observation counts of every residue mod 4);
the 4-slot tree of tests/test_gpu_k4_fold.py (the form does not apply: PLK_INFO_LL_PAIRMUL 0, the folded stream runs);
nchar 4, 5, 16 with C 1, 4 and S 1, 129, 300; the site count of tests/test_gpu_k4_fold.py at which some waves walk two units;
the + 512 bit toggled on a live engine against fresh ones; BASELINE config 3 at S = 300 (20 PAIR ops a category).
Which handlers a stream dispatches is pinned on the CPU (tests/pairmulcheck_main.cpp).
"""
import numpy as np
import pytest

from helpers import rel_err
from test_gpu_k4_stream import _codes, _workload, caterpillar
from test_gpu_k4_fold import _bal_shape, _cat_shape, _fold_info, _nested, _oracle_ll, _shape_edges

pytestmark = pytest.mark.gpu

TOL, SUM_TOL = 1e-12, 1e-13
PAIRED, FOLDED, TILE, TILE_SMALL = 1, 1 + 512, 6, 5
FUSED = 1


@pytest.fixture(scope="module")
def eng():
    from phyly_amd import engine as E
    e = E.Engine(0)
    yield e
    e.set_option(E.OPT_PAIR_TABLES, 1)
    e.close()


def _run(eng, option):
    from phyly_amd import engine as E
    eng.set_option(E.OPT_PAIR_TABLES, option)
    site, (hi, lo) = eng.ll()
    what = (eng.info(E.INFO_LL_KERNEL), eng.info(E.INFO_LL_VARIANT), eng.info(E.INFO_LL_FORM), eng.info(E.INFO_LL_FOLD),
            eng.info(E.INFO_LL_PAIRMUL))
    return site.copy(), float(hi), float(lo), what


def _three(eng, tag, want, paired=True):
    """default, + 512, tile: the comparisons of the module docstring; -> (PAIR ops of a category, PLK_INFO_LL_FOLD as a dict)"""
    p = _run(eng, PAIRED)
    f = _run(eng, FOLDED)
    t = _run(eng, TILE)
    if t[3][1] != 6:
        t = _run(eng, TILE_SMALL)
    assert p[3][:3] == (FUSED, 6, 1) and f[3][:3] == (FUSED, 6, 1) and t[3][:3] == (FUSED, 6, 0), (tag, p[3], f[3], t[3])
    # the fold's description does not depend on the form; + 512 and the tile kernel report no pair products
    assert p[3][3] == f[3][3] and f[3][4] == 0 and t[3][4] == 0 and t[3][3] == 0, (tag, p[3], f[3], t[3])
    info = _fold_info(p[3][3])
    assert info["folded"] and info["held"], (tag, info)
    assert (p[3][4] & 1) == (1 if paired else 0) and (paired or p[3][4] == 0), (tag, p[3])
    npair = (p[3][4] >> 8) & 0xFFFF
    assert np.all(np.isfinite(t[0])), tag
    assert np.array_equal(p[0].view(np.uint64), f[0].view(np.uint64)), tag
    assert np.array_equal(p[0].view(np.uint64), t[0].view(np.uint64)), tag
    hl = lambda r: np.array([r[1], r[2]]).view(np.uint64).tolist()
    assert hl(p) == hl(f), (tag, p[1:3], f[1:3])
    rel = abs((p[1] + p[2]) - (t[1] + t[2])) / abs(t[1] + t[2])
    print("%s: sum %.17g, against the tile kernel rel %.3g, PAIR ops %d, fold %s" % (tag, p[1] + p[2], rel, npair, info))
    assert rel <= SUM_TOL, (tag, rel)
    for name, r in (("pair products", p), ("folded", f), ("tile", t)):
        err = rel_err(r[0], want)
        assert err <= TOL, (tag, name, err)
    return npair, info


def _case(eng, oracle, wl, S, tag, seed=3, paired=True):
    wl.setup_engine(eng)
    codes = _codes(wl, S, seed=seed)
    eng.set_patterns_codes(codes, wl.defs)
    eng.set_site_weights(None)
    return _three(eng, "%s S=%d" % (tag, S), _oracle_ll(oracle, wl, codes), paired)


def test_smallest_trees(eng, oracle):
    """(cherry, leaf): a pair table and a leaf, one PAIR and nothing else observed; ((cherry), (cherry)): two pair tables"""
    for S in (1, 129):
        npair, _ = _case(eng, oracle, _workload(_shape_edges(((0, 0), 0)), seed=3), S, "three leaves")
        assert npair == 1
        npair, _ = _case(eng, oracle, _workload(_shape_edges(((0, 0), (0, 0))), seed=4), S, "four leaves")
        assert npair == 1


@pytest.mark.parametrize("nchar", [4, 5, 16])
@pytest.mark.parametrize("C", [1, 4])
def test_site_counts(eng, oracle, nchar, C):
    """one partly filled unit, two units, a third unit whose second site half is partly filled"""
    wl = _workload(caterpillar(8), C=C, nchar=nchar, seed=50 + nchar + C)
    for S in (1, 129, 300):
        npair, info = _case(eng, oracle, wl, S, "nchar%d C%d" % (nchar, C), seed=nchar)
        # 7 observations: one chunk rotation; the cherry's table and the leaf above it are adjacent look-ups
        assert npair >= 1 and info["adv0"] + info["adv1"] == 1


@pytest.mark.parametrize("lead", [0, 1])
def test_parities_and_advances(eng, oracle, lead):
    """3 .. 12 leaves, caterpillar and balanced, alone and as the subtree next to one more leaf under the root"""
    pairs = set()
    for n in range(3, 13):
        for kind, shape in (("caterpillar", _cat_shape(n)), ("balanced", _bal_shape(n))):
            wl = _workload(_shape_edges((0, shape) if lead else shape), seed=100 + n + 50 * lead)
            npair, _ = _case(eng, oracle, wl, 129, "%s%d lead%d" % (kind, n, lead), seed=n)
            pairs.add(npair)
    # without the extra leaf a program starts with two adjacent look-ups (the first cherry's table, then its sibling leaf or
    # its sibling cherry's table); the balanced trees have such nodes further up as well
    assert lead or min(pairs) >= 1, pairs
    assert max(pairs) >= 2, pairs


def test_four_slots_fall_back(eng, oracle):
    """the 4-slot tree keeps the folded stream on k_ll_fused4_v4s under the default option, and says so"""
    from phyly_amd import engine as E
    npair, info = _case(eng, oracle, _workload(_nested(), seed=39), 129, "nested39", paired=False)
    assert npair == 0 and info["folded"] and eng.info(E.INFO_STACK_SLOTS) == 4


def test_config3(eng, oracle):
    from phyly_amd import synth
    wl = synth.Workload(3)
    wl.setup_engine(eng)
    codes = wl.simulate(300)
    eng.set_patterns_codes(codes, wl.defs)
    eng.set_site_weights(None)
    npair, info = _three(eng, "config 3 S=300", _oracle_ll(oracle, wl, codes))
    assert npair == 20 and (info["adv0"], info["adv1"]) == (8, 8) and info["scale_left"] == 2


def test_two_units_per_wave(eng, oracle):
    """the site count of tests/test_gpu_k4_fold.py: on a GPU of up to 304 CUs some waves walk two units (the held chunks of
    the next unit travel during the first one's epilogue) and the others one.  The alignment repeats the columns of a small
    one, so the oracle is asked for those only."""
    wl = _workload(caterpillar(8), seed=77)
    wl.setup_engine(eng)
    S0 = 128 * 12 * 2 + 5
    block = _codes(wl, S0, seed=9)
    want = _oracle_ll(oracle, wl, block)
    S = 304 * 12 * 128 + S0
    codes = np.ascontiguousarray(np.tile(block, (1, (S + S0 - 1) // S0))[:, :S])
    eng.set_patterns_codes(codes, wl.defs)
    eng.set_site_weights(None)
    _three(eng, "units S=%d" % S, np.tile(want, (S + S0 - 1) // S0)[:S])


def test_stale_plan_pair_bit():
    """the + 512 bit (and + 64, which implies it) toggled on a live engine: after each toggle it answers bit for bit as an
    engine created with that option and reports the same kernel, variant, form, fold and pair products"""
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
        for option in (1, 1 + 512, 1, 7 + 512, 7, 1 + 64, 1, 6, 1 + 512, 1):
            got, want = _run(live, option), fresh(option)
            assert got[3] == want[3], (option, got[3], want[3])
            assert np.array_equal(got[0].view(np.uint64), want[0].view(np.uint64)) and got[1:3] == want[1:3], option
            seen.add((got[3][2], got[3][4] & 1))
        assert seen == {(1, 1), (1, 0), (0, 0)}, seen                # pair products, streamed without them, the tile kernel
    finally:
        live.close()
