"""GPU: the streamed k = 4 kernel (k_ll_fused4_v4s) with the FOLDED op stream and the unit's first chunks held across the
categories (the default, PLK_OPT_PAIR_TABLES 1), against the same kernel without either (+ 64: the checked stream as it
is built, every category requesting the first chunks itself) and against the 1536-site tile kernel (6, or 5 where 6 does
not fit).

The three run the same instruction sequence per site on the same operands, so site_ll is compared on its uint64 view.
Folded and unfolded give the same wave the same units in the same order: {hi, lo} of the sum equal bit for bit.  The tile
kernel sums in another order: hi + lo within 1e-13 relative.  All three against the oracle (binary128) at 1e-12.

Shapes: site counts around the 128-site unit with nchar 4, 5, 16 and C 1, 4; caterpillars and balanced trees of 3 .. 12
leaves (no, one and two folded ADVANCEs of both kinds); trees with SCALE ops such that every MATVEC + POPMUL + SCALE
handler (slots 0 .. 3) is dispatched and some SCALE keeps a dispatch of its own (PLK_INFO_LL_FOLD reports what the uploaded
stream holds); the stack-slot trees of tests/test_gpu_k4_variants.py; the + 64 / + 128 / + 256 bits toggled on a live engine
against fresh ones; a site count at which some waves walk two units and others one (next unit's chunks, and the guard that
requests nothing past the last unit).
"""
import numpy as np
import pytest

from helpers import k4_workload, oracle_model, rel_err
from test_gpu_k4_stream import _codes, _workload, caterpillar

pytestmark = pytest.mark.gpu

TOL, SUM_TOL = 1e-12, 1e-13
FOLDED, UNFOLDED, TILE, TILE_SMALL = 1, 1 + 64, 6, 5
FUSED = 1


def _fold_info(v):
    """PLK_INFO_LL_FOLD -> dict"""
    return dict(folded=bool(v & 1), held=bool(v & 2), scale_slots=(v >> 4) & 15, scale_left=(v >> 8) & 255, adv0=(v >> 16) & 255, adv1=(v >> 24) & 127)


def _shape_edges(shape):
    """nested tuples (0 = a leaf) -> edges; leaves 0 .. T-1 in order of appearance, internal nodes after them"""
    def count(s):
        return 1 if s == 0 else sum(count(c) for c in s)
    edges, nxt = [], [0, count(shape)]

    def walk(s):
        if s == 0:
            nxt[0] += 1
            return nxt[0] - 1
        kids = [walk(c) for c in s]
        me = nxt[1]
        nxt[1] += 1
        edges.extend([me, k] for k in kids)
        return me
    walk(shape)
    return edges


def _cat_shape(n):
    s = (0, 0)
    for _ in range(2, n):
        s = (s, 0)
    return s


def _balanced(n):
    from phyly_amd import synth
    return synth.make_tree(n, "balanced", 1)


def _bal_shape(n):
    return 0 if n == 1 else (_bal_shape(n - n // 2), _bal_shape(n // 2))


def _nested():
    """39 leaves, 4 stack slots: joins of two 5-leaf caterpillars (9 + 9 edge factors: a SCALE right after the MATVEC +
    POPMUL of the join) evaluated with 0, 1, 2 and 3 vectors waiting"""
    five = (_cat_shape(5), _cat_shape(5))
    return _shape_edges((_bal_shape(16), (_bal_shape(8), (five, five))))


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
    what = (eng.info(E.INFO_LL_KERNEL), eng.info(E.INFO_LL_VARIANT), eng.info(E.INFO_LL_FORM), eng.info(E.INFO_LL_FOLD))
    return site.copy(), float(hi), float(lo), what


def _three(eng, tag, want=None, streamed=True):
    """default, + 64, tile: the comparisons of the module docstring; -> PLK_INFO_LL_FOLD of the default as a dict"""
    f = _run(eng, FOLDED)
    u = _run(eng, UNFOLDED)
    t = _run(eng, TILE)
    if streamed and t[3][1] != 6:
        t = _run(eng, TILE_SMALL)
    info = _fold_info(f[3][3])
    if streamed:
        assert f[3][:3] == (FUSED, 6, 1) and u[3][:3] == (FUSED, 6, 1) and t[3][:3] == (FUSED, 6, 0), (tag, f[3], u[3], t[3])
        assert info["folded"] and info["held"], (tag, info)
        assert u[3][3] == 0 and t[3][3] == 0, (tag, u[3], t[3])
    else:
        assert f[3] == u[3] == t[3] and f[3][2] == 0 and f[3][3] == 0, (tag, f[3], u[3], t[3])
    assert np.all(np.isfinite(t[0])), tag
    assert np.array_equal(f[0].view(np.uint64), u[0].view(np.uint64)), tag
    assert np.array_equal(f[0].view(np.uint64), t[0].view(np.uint64)), tag
    hl = lambda r: np.array([r[1], r[2]]).view(np.uint64).tolist()
    assert hl(f) == hl(u), (tag, f[1:3], u[1:3])
    rel = abs((f[1] + f[2]) - (t[1] + t[2])) / abs(t[1] + t[2])
    print("%s: sum %.17g, against the tile kernel rel %.3g, fold %s" % (tag, f[1] + f[2], rel, info))
    assert rel <= SUM_TOL, (tag, rel)
    if want is not None:
        for name, r in (("folded", f), ("unfolded", u), ("tile", t)):
            err = rel_err(r[0], want)
            assert err <= TOL, (tag, name, err)
    return info


def _oracle_ll(oracle, wl, codes):
    m, w = oracle_model(oracle, wl, codes)
    want, _ = oracle.site_ll(m, w, codes=np.ascontiguousarray(codes.T), defs=wl.defs, precise=2)
    return want


def _case(eng, oracle, wl, S, tag, seed=3, streamed=True):
    wl.setup_engine(eng)
    codes = _codes(wl, S, seed=seed)
    eng.set_patterns_codes(codes, wl.defs)
    eng.set_site_weights(None)
    return _three(eng, "%s S=%d" % (tag, S), _oracle_ll(oracle, wl, codes), streamed)


@pytest.mark.parametrize("nchar", [4, 5, 16])
@pytest.mark.parametrize("C", [1, 4])
def test_site_counts(eng, oracle, nchar, C):
    """one partly filled unit, two units, a third unit whose second site half is partly filled"""
    wl = _workload(caterpillar(8), C=C, nchar=nchar, seed=50 + nchar + C)
    for S in (1, 129, 300):
        info = _case(eng, oracle, wl, S, "nchar%d C%d" % (nchar, C), seed=nchar)
        assert info["adv0"] + info["adv1"] == 1                   # 7 observations: one chunk rotation


def test_advance_boundaries(eng, oracle):
    """3 .. 12 leaves: the number of observation ops takes every residue mod 4; streams with no, one, and two folded
    ADVANCEs, of both kinds"""
    seen = set()
    for n in range(3, 13):
        for kind, edges in (("caterpillar", caterpillar(n)), ("balanced", _balanced(n))):
            wl = _workload(edges, seed=100 + n)
            info = _case(eng, oracle, wl, 129, "%s%d" % (kind, n), seed=n)
            seen.add((info["adv0"], info["adv1"]))
    assert (0, 0) in seen and (1, 0) in seen and any(a >= 1 and b >= 1 for a, b in seen), seen


def test_scale_folds(eng, oracle):
    """trees with SCALE ops.  The 64-leaf balanced tree needs 5 stack slots, which the pair-table kernels do not take: the
    three options then run one and the same kernel and agree trivially; it is kept because it belongs to the list.  The
    other trees run the streamed form; between them every MATVEC + POPMUL + SCALE handler is dispatched and a SCALE (after
    the MATVEC + TIP_MUL of a caterpillar) keeps its own dispatch."""
    slots, left = 0, 0
    info = _case(eng, oracle, _workload(caterpillar(40), seed=40), 129, "caterpillar40")
    assert info["scale_left"] >= 1 and info["adv0"] >= 2 and info["adv1"] >= 2
    slots |= info["scale_slots"]; left += info["scale_left"]
    _case(eng, oracle, _workload(_balanced(64), seed=64), 129, "balanced64", streamed=False)
    info = _case(eng, oracle, _workload(_balanced(32), seed=32), 129, "balanced32")
    slots |= info["scale_slots"]
    info = _case(eng, oracle, _workload(_nested(), seed=39), 129, "nested39")
    slots |= info["scale_slots"]
    from phyly_amd import synth
    wl = synth.Workload(3)
    wl.setup_engine(eng)
    codes = wl.simulate(300)
    eng.set_patterns_codes(codes, wl.defs)
    eng.set_site_weights(None)
    info = _three(eng, "config 3 S=300", _oracle_ll(oracle, wl, codes))
    assert (info["adv0"], info["adv1"]) == (8, 8) and info["scale_left"] == 2
    slots |= info["scale_slots"]
    assert slots == 0xF and left >= 1, (slots, left)


@pytest.mark.parametrize("model", ["balanced32", "irregular"])
def test_stack_slots(eng, oracle, model):
    """the models of tests/test_gpu_k4_variants.py the pair-table kernels take: 4 slots (PUSH and POPMUL of slots 0 .. 3) and
    the irregular tree (unary node, multifurcations, data on internal nodes, a rate-0 category)"""
    from phyly_amd import engine as E
    wl = k4_workload(model)
    wl.setup_engine(eng)
    codes = wl.simulate(257)
    eng.set_patterns_codes(codes, wl.defs)
    eng.set_site_weights(None)
    _three(eng, model, _oracle_ll(oracle, wl, codes))
    assert eng.info(E.INFO_STACK_SLOTS) == (4 if model == "balanced32" else 1)


def test_two_units_per_wave(eng, oracle):
    """S = 128 * 12 * 2 + 5 (two units for every wave of one workgroup, were there one workgroup: the launch spreads them
    over three), and that many sites past 304 workgroups' worth of units: on a GPU of up to 304 CUs some waves walk two
    units (the next unit's chunks are requested during the first one's epilogue) and the others one (nothing is requested
    past the last unit).  The large alignment repeats the columns of the small one, so one oracle call serves both."""
    wl = _workload(caterpillar(8), seed=77)
    wl.setup_engine(eng)
    S0 = 128 * 12 * 2 + 5
    block = _codes(wl, S0, seed=9)
    want = _oracle_ll(oracle, wl, block)
    for S in (S0, 304 * 12 * 128 + S0):
        codes = np.ascontiguousarray(np.tile(block, (1, (S + S0 - 1) // S0))[:, :S])
        eng.set_patterns_codes(codes, wl.defs)
        eng.set_site_weights(None)
        _three(eng, "units S=%d" % S, np.tile(want, (S + S0 - 1) // S0)[:S])


def test_stale_plan_fold_bits():
    """the + 64, + 128 and + 256 bits toggled on a live engine: after each toggle it answers bit for bit as an engine
    created with that option and reports the same kernel, variant, form and fold"""
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
        for option in (1, 1 + 64, 1, 1 + 128, 1 + 256, 7 + 64, 7, 6, 1 + 64, 6 + 64, 1):
            got, want = _run(live, option), fresh(option)
            assert got[3] == want[3], (option, got[3], want[3])
            assert np.array_equal(got[0].view(np.uint64), want[0].view(np.uint64)) and got[1:3] == want[1:3], option
            seen.add(got[3][3] & 3)
        assert seen == {0, 1, 2, 3}, seen                            # neither, fold only, held chunks only, both
    finally:
        live.close()
