"""GPU: the streamed k = 4 kernel where a wave walks several units, and its barrier default.

With one workgroup per CU a wave has a second unit only beyond 393 216 sites, so the paths "the next unit's first chunks
were requested during the previous unit", "a wave's last pass is partial or missing" and "the wrap from a phase's last unit
to the next phase's first" are reached here by capping the launch at 1 and 2 workgroups (PLK_OPT_STREAM_GRID): S = 12 x 128 x
3 + 77 = 4685 is three full passes and a partial fourth for some waves and none for others (1 workgroup), or one full pass
and a partial second (2).  Also S = 1 (one wave has a unit), 129 (two) and 12 x 128 (one full pass, nobody has a next unit).

The waves of a workgroup meet before every category by default, except where one category is resident at a time (one rate
category, a group per category): there they never meet (plk_v4s_auto_sync).  Every run is made with the default and with the
barrier forced before every unit (+ 16), never (+ 32) and before every category (+ 65536): a site's arithmetic does not
depend on it, so site_ll is compared on its uint64 view across all of them and across the workgroup caps, {hi, lo} of the sum
bit for bit across the barrier variants of one cap (the same waves walk the same units), and site_ll against the oracle
(binary128) at 1e-12.  PLK_INFO_LL_BARRIER, which the launch sets from the argument it hands the kernel, must report the forced
mode under each bit and, for the default, "never, chosen" exactly where the reported plan leaves one category resident at a time
(C = 1, or as many groups as categories) and "every category, chosen" elsewhere (all categories resident, two groups of two).

Shapes: a 12-leaf caterpillar (3 stack slots: the pair-product text, the only one with phases) and the 39-leaf nested tree of
tests/test_gpu_k4_fold.py (4 slots: the folded text), C = 1 and 4, the categories forced into 1, 2 and C groups, the four-leaf
form forced and forbidden, site weights with zeros, the sum without site_ll, the options set on a live engine, and BASELINE
config 3's tree under the default plan.  Which plans run without the barrier is pinned on the CPU (tests/synccheck_main.cpp).
"""
import numpy as np
import pytest

from helpers import rel_err
from test_gpu_k4_stream import _weights, _workload, caterpillar
from test_gpu_k4_fold import _nested, _oracle_ll
from test_gpu_k4_quad import _qcodes

pytestmark = pytest.mark.gpu

TOL = 1e-12
QUAD, NEVER = 1 + 16384, 1 + 32768
ONE_GROUP, TWO_GROUPS, GROUP_PER_CATEGORY = 4096, 4096 + 8192, 8192
EVERY_UNIT, NO_BARRIER, EVERY_CATEGORY = 16, 32, 65536
BARRIER_NEVER, BARRIER_UNIT, BARRIER_CATEGORY, BARRIER_CHOSEN = 1, 2, 3, 16          # PLK_INFO_LL_BARRIER
BIG = 12 * 128 * 3 + 77
SIZES = (BIG, 1, 129, 12 * 128)
TREES = {"pair": lambda C: _workload(caterpillar(12), C=C, seed=71 + C), "folded": lambda C: _workload(_nested(), C=C, seed=73 + C)}


@pytest.fixture(scope="module")
def eng():
    from phyly_amd import engine as E
    e = E.Engine(0)
    yield e
    e.set_option(E.OPT_PAIR_TABLES, 1)
    e.set_option(E.OPT_STREAM_GRID, 0)
    e.close()


_reference = {}


def _shape(oracle, text, C):
    """workload, codes of the largest site count (smaller counts take its first sites) and the oracle's site_ll, computed once"""
    if (text, C) not in _reference:
        wl = TREES[text](C)
        codes = _qcodes(wl, BIG, 5 + C)
        want = _oracle_ll(oracle, wl, codes)
        want.setflags(write=False)
        _reference[(text, C)] = (wl, codes, want)
    return _reference[(text, C)]


def _run(eng, option, grid, per_site=True):
    from phyly_amd import engine as E
    eng.set_option(E.OPT_STREAM_GRID, grid)
    eng.set_option(E.OPT_PAIR_TABLES, option)
    site, (hi, lo) = eng.ll(per_site=per_site)
    what = dict(kernel=eng.info(E.INFO_LL_KERNEL), form=eng.info(E.INFO_LL_FORM), fold=eng.info(E.INFO_LL_FOLD) & 3, pairmul=eng.info(E.INFO_LL_PAIRMUL) & 1,
                groups=(eng.info(E.INFO_LL_TRIPLE) >> 4) & 15, quad=eng.info(E.INFO_LL_QUAD) & 1)
    what["barrier"] = eng.info(E.INFO_LL_BARRIER)
    what["C"] = eng.info(E.INFO_CATEGORIES)
    return (site.copy() if per_site else None), np.array([float(hi), float(lo)]).view(np.uint64).tolist(), what


def _barrier_variants(eng, option, grid, tag, text, want=None, per_site=True):
    """the default, + 16, + 32, + 65536: the same plan, equal bits, the barrier mode reported -> the default's run"""
    runs = [_run(eng, option + b, grid, per_site) for b in (0, EVERY_UNIT, NO_BARRIER, EVERY_CATEGORY)]
    first = runs[0]
    # categories resident at a time, from the plan the run reports (no groups reported: no tables, all of them resident)
    resident = -(-first[2]["C"] // max(first[2]["groups"], 1))
    modes = [r[2].pop("barrier") for r in runs]
    assert modes == [BARRIER_CHOSEN + (BARRIER_NEVER if resident == 1 else BARRIER_CATEGORY), BARRIER_UNIT, BARRIER_NEVER, BARRIER_CATEGORY], (tag, modes, first[2])
    for r in runs:
        assert r[2]["kernel"] == 1 and r[2]["form"] == 1 and r[2]["fold"] == 3 and r[2]["pairmul"] == (1 if text == "pair" else 0), (tag, r[2])
        assert r[2] == first[2] and r[1] == first[1], (tag, r[2], first[2], r[1], first[1])
        if per_site:
            assert np.array_equal(r[0].view(np.uint64), first[0].view(np.uint64)), tag
    if per_site and want is not None:
        err = rel_err(first[0], want)
        print("%s: rel err %.3g" % (tag, err))
        assert np.all(np.isfinite(first[0])) and err <= TOL, (tag, err)
    return first


@pytest.mark.parametrize("C", [1, 4])
@pytest.mark.parametrize("text", ["pair", "folded"])
def test_several_units_a_wave(eng, oracle, text, C):
    wl, codes, want = _shape(oracle, text, C)
    wl.setup_engine(eng)
    for S in SIZES:
        eng.set_patterns_codes(np.ascontiguousarray(codes[:, :S]), wl.defs)
        eng.set_site_weights(None)
        uncapped = _run(eng, 1, 0)
        # every combination at the site count with several passes, the two ends of the range at the others
        combos = [(q, g) for q in (QUAD, NEVER) for g in (ONE_GROUP, TWO_GROUPS, GROUP_PER_CATEGORY)] if S == BIG else [(QUAD, GROUP_PER_CATEGORY), (NEVER, ONE_GROUP)]
        seen = set()
        for grid in (1, 2):
            for quad, groups in combos:
                tag = "%s C%d S=%d grid %d option %d" % (text, C, S, grid, quad + groups)
                r = _barrier_variants(eng, quad + groups, grid, tag, text, want[:S])
                assert np.array_equal(r[0].view(np.uint64), uncapped[0].view(np.uint64)), tag
                seen.add((r[2]["quad"], r[2]["groups"]))
        if S == BIG:
            # phases exist in the pair-product instantiation only; a forbidden four-leaf form leaves no table at all here
            assert (1, 1) in seen and any(q == 0 for q, _ in seen), seen
            assert ((1, C) in seen and (1, min(2, C)) in seen) if text == "pair" else all(g <= 1 for _, g in seen), seen


@pytest.mark.parametrize("text", ["pair", "folded"])
def test_weights_with_zeros_and_sum_only(eng, oracle, text):
    wl, codes, want = _shape(oracle, text, 4)
    wl.setup_engine(eng)
    eng.set_patterns_codes(codes, wl.defs)
    eng.set_site_weights(_weights(BIG))
    try:
        for grid in (1, 2):
            for option in (QUAD + GROUP_PER_CATEGORY, NEVER + TWO_GROUPS):
                tag = "%s weights grid %d option %d" % (text, grid, option)
                site = _barrier_variants(eng, option, grid, tag, text, want)
                summed = _barrier_variants(eng, option, grid, tag + " sum only", text, per_site=False)
                assert summed[1] == site[1], tag
    finally:
        eng.set_site_weights(None)


def test_options_on_a_live_engine(oracle):
    """PLK_OPT_STREAM_GRID and the barrier bits set after an evaluation: the next one answers bit for bit as a fresh engine
    with these options and reports the same plan"""
    from phyly_amd import engine as E
    wl, codes, _ = _shape(oracle, "pair", 4)

    def fresh(option, grid):
        e = E.Engine(0)
        try:
            wl.setup_engine(e)
            e.set_patterns_codes(codes, wl.defs)
            return _run(e, option, grid)
        finally:
            e.close()

    live = E.Engine(0)
    try:
        wl.setup_engine(live)
        live.set_patterns_codes(codes, wl.defs)
        site0, _ = live.ll()
        seen = set()
        for option, grid in ((1, 0), (1, 1), (1 + NO_BARRIER, 1), (QUAD + GROUP_PER_CATEGORY, 2), (QUAD + GROUP_PER_CATEGORY + EVERY_CATEGORY, 2), (1, 2), (1, 0)):
            got, want = _run(live, option, grid), fresh(option, grid)
            assert got[2] == want[2], (option, grid, got[2], want[2])
            assert np.array_equal(got[0].view(np.uint64), want[0].view(np.uint64)) and got[1] == want[1], (option, grid)
            assert np.array_equal(got[0].view(np.uint64), site0.view(np.uint64)), (option, grid)
            seen.add((grid, got[2]["groups"]))
        # (workgroup cap, groups reported): the default takes three- and four-leaf tables where every wave makes at least
        # PLK_V4T_MIN_PASSES = 3 passes: 37 units are 4 passes of the 12 waves of one workgroup, 2 of 24 waves, 1 of every CU's
        assert seen == {(0, 0), (1, 1), (2, 0), (2, 4)}, seen
    finally:
        live.close()


def test_config3_default_plan(eng, oracle):
    from phyly_amd import synth
    wl = synth.Workload(3)
    wl.setup_engine(eng)
    codes = wl.simulate(BIG)
    eng.set_patterns_codes(codes, wl.defs)
    eng.set_site_weights(None)
    want = _oracle_ll(oracle, wl, codes)
    sites = [_barrier_variants(eng, 1, grid, "config 3 S=%d grid %d" % (BIG, grid), "pair", want)[0] for grid in (0, 1, 2)]
    assert np.array_equal(sites[0].view(np.uint64), sites[1].view(np.uint64)) and np.array_equal(sites[0].view(np.uint64), sites[2].view(np.uint64))
