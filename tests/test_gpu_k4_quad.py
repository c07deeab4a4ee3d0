"""GPU: four-leaf tables in the streamed k = 4 kernel (PLK_OPT_PAIR_TABLES + 16384: a node that is not the root, with four
leaves below it as ((cherry, leaf), leaf) or (cherry, cherry), each leaf taking at most 4 of the nchar codes in the uploaded
patterns, is with the edge above it one look-up of a 256-row table indexed by the leaves' code ranks) against the same engine
under + 32768 (never) and under + 2048 (neither four-leaf nor three-leaf tables).

A row of a four-leaf table is the handlers' own fp64 sequence on the handlers' own operands and a site's category terms are
added in the same order whatever the groups, so site_ll is compared on its uint64 view and {hi, lo} of the sum bit for bit
(the same waves walk the same units).  All of them against the oracle (binary128) at 1e-12.

Shapes, the smallest that can go wrong: the two five-leaf shapes at S = 1, 129, 300; what follows the absorbed product (PUSH,
POPMUL, TIP_MUL, MATVEC); nchar 4, 5 and 16 with at most 4 occurring codes per leaf, scattered over the definitions and
different from leaf to leaf, with C 1, 3, 4 forced into 1, 2 and C groups; a leaf with 5 occurring codes (no four-leaf table,
the three-leaf table below it instead) and a leaf with a single one; site weights; the sum without site_ll; a site of
likelihood zero and a rate-0 category; the 40-leaf caterpillar the program rescales; BASELINE config 3 at S = 300 (counts
set against the plan's unit budget); the option toggled on a live engine against fresh ones; patterns replaced on a live
engine, first fully observed, then with missing data at some leaves, against fresh engines.  The default at these site
counts does not take the form.  Which nodes qualify, the rank tables, the replay checks and the rows are pinned on the CPU
(tests/quadcheck_main.cpp).
"""
import numpy as np
import pytest

from helpers import rel_err, tree_workload
from test_gpu_k4_stream import _weights, _workload, caterpillar
from test_gpu_k4_fold import _oracle_ll, _shape_edges

pytestmark = pytest.mark.gpu

TOL = 1e-12
DEFAULT, QUAD, NEVER, PLAIN, TRIPLE = 1, 1 + 16384, 1 + 32768, 1 + 2048, 1 + 1024
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
            eng.info(E.INFO_LL_TRIPLE), eng.info(E.INFO_LL_QUAD))
    return (site.copy() if per_site else None), float(hi), float(lo), what


def _info(what):
    t, q = what[4], what[5]
    assert q == 0 or (q & 1 and t & 1), what
    return dict(quads=(q >> 8) & 0xFFFF, groups=(t >> 4) & 15, triples=(t >> 8) & 0xFFFF)


def _hl(r):
    return np.array([r[1], r[2]]).view(np.uint64).tolist()


def _qcodes(wl, S, seed, allowed=None):
    """codes[N][S]: leaf number i (in node order) draws from allowed(i), by default from 0 .. 3, and takes every one of them
    where S allows; internal nodes carry the all-ones definition"""
    rng = np.random.default_rng([seed, S])
    miss = min(4, wl.nchar - 1)
    codes = np.full((wl.N, S), miss, dtype=np.uint8)
    leaf = wl.indptr[1:] == wl.indptr[:-1]
    i = 0
    for a in range(wl.N):
        if not leaf[a]:
            continue
        pool = np.array(allowed(i) if allowed else [0, 1, 2, 3], dtype=np.uint8)
        codes[a] = pool[rng.integers(0, len(pool), S)]
        codes[a, :min(S, len(pool))] = pool[:min(S, len(pool))]
        i += 1
    return codes


def _compare(eng, tag, want, groups=0):
    """+ 16384 (+ groups), + 32768, + 2048 and the default: the comparisons of the module docstring -> counts of the forced run"""
    q = _run(eng, QUAD + groups)
    n = _run(eng, NEVER)
    p = _run(eng, PLAIN)
    d = _run(eng, DEFAULT)
    for r in (q, n, p, d):
        assert r[3][:3] == (FUSED, 6, 1), (tag, r[3])
    assert n[3][5] == 0 and p[3][5] == 0 and p[3][4] == 0, (tag, n[3], p[3])
    assert d[3][5] == 0 and d[3][4] == 0, (tag, d[3])              # the default at these site counts
    assert np.all(np.isfinite(p[0]) | np.isneginf(p[0])), tag
    assert np.array_equal(q[0].view(np.uint64), n[0].view(np.uint64)), tag
    assert np.array_equal(q[0].view(np.uint64), p[0].view(np.uint64)), tag
    assert _hl(q) == _hl(n) == _hl(p) == _hl(d), (tag, q[1:3], n[1:3], p[1:3])
    if want is not None:
        keep = np.isfinite(want)
        for name, r in (("four-leaf tables", q), ("never", n), ("without", p)):
            err = rel_err(r[0][keep], want[keep])
            print("%s %s: rel err %.3g" % (tag, name, err))
            assert err <= TOL, (tag, name, err)
    info = _info(q[3])
    print("%s: sum %.17g, %s" % (tag, q[1] + q[2], info))
    return info


def _case(eng, oracle, wl, S, tag, seed=3, groups=0, allowed=None):
    wl.setup_engine(eng)
    codes = _qcodes(wl, S, seed, allowed)
    eng.set_patterns_codes(codes, wl.defs)
    eng.set_site_weights(None)
    return _compare(eng, "%s S=%d" % (tag, S), _oracle_ll(oracle, wl, codes), groups)


SHAPE_A, SHAPE_B = ((((0, 0), 0), 0), 0), (((0, 0), (0, 0)), 0)


@pytest.mark.parametrize("shape", ["A", "B"])
def test_five_leaf_shapes(eng, oracle, shape):
    wl = _workload(_shape_edges(SHAPE_A if shape == "A" else SHAPE_B), seed=3)
    for S in (1, 129, 300):
        assert _case(eng, oracle, wl, S, "shape " + shape) == dict(quads=1, groups=1, triples=0)


def test_root_is_not_absorbed(eng, oracle):
    """(((0, 0), 0), 0): the four-leaf node is the root; the three-leaf node below it is a table (+ 16384 implies + 1024)"""
    info = _case(eng, oracle, _workload(_shape_edges((((0, 0), 0), 0)), seed=5), 129, "root")
    assert info == dict(quads=0, groups=1, triples=1)


FOLLOWERS = {
    "TIP_MUL": SHAPE_A,                                 # the parent's next child is a leaf
    "MATVEC": ((((((0, 0), 0), 0),), 0), 0),            # a unary node above: the next op is the product of its edge
    "PUSH": ((((0, 0), 0), 0), (0, 0)),                 # first of two internal children
    "POPMUL": (((0, 0), 0), (((0, 0), 0), 0)),          # second of two internal children (the first one is a three-leaf table)
}


@pytest.mark.parametrize("follower", list(FOLLOWERS))
def test_what_follows_the_absorbed_product(eng, oracle, follower):
    for groups in (ONE_GROUP, TWO_GROUPS):
        info = _case(eng, oracle, _workload(_shape_edges(FOLLOWERS[follower]), seed=11), 129, follower, groups=groups)
        assert info["quads"] == 1 and info["groups"] == (1 if groups == ONE_GROUP else 2), info


SCATTERED = {4: [[0, 2], [1, 3], [0, 1, 2, 3], [2]],
             5: [[0, 2, 4], [1, 3], [0, 1, 2, 4], [3, 4]],
             16: [[1, 5, 9, 15], [0, 7, 8], [2, 3, 14, 15], [6, 10, 11, 12]]}


@pytest.mark.parametrize("nchar", [4, 5, 16])
@pytest.mark.parametrize("C", [1, 3, 4])
def test_scattered_codes_and_groups(eng, oracle, nchar, C):
    """occurring codes scattered over the definitions, another subset at every leaf, code 0 missing at most leaves (the padded
    sites of the last unit must land on rank 0); 8 leaves: one shape-A table, with both shapes' tree below"""
    wl = _workload(caterpillar(8), C=C, nchar=nchar, seed=60 + nchar + C)
    allowed = lambda i: SCATTERED[nchar][i % 4]
    for groups, ngroups in ((ONE_GROUP, 1), (TWO_GROUPS, min(2, C)), (GROUP_PER_CATEGORY, C)):
        for S in ((1, 129, 300) if groups == ONE_GROUP else (129,)):
            info = _case(eng, oracle, wl, S, "nchar%d C%d groups%d" % (nchar, C, ngroups), seed=nchar, groups=groups, allowed=allowed)
            assert info == dict(quads=1, groups=ngroups, triples=0), info


def test_five_codes_at_a_leaf_and_a_single_code(eng, oracle):
    wl = _workload(_shape_edges(SHAPE_A), seed=17)
    # the leaf beside the three-leaf node takes all 5 codes: nothing absorbed at d, the three-leaf node is a table
    info = _case(eng, oracle, wl, 300, "five codes", allowed=lambda i: [0, 1, 2, 3, 4] if i == 3 else [0, 1, 2, 3])
    assert info == dict(quads=0, groups=1, triples=1)
    # a leaf of the cherry takes 5: no three-leaf candidate depends on that, so the three-leaf table is still taken
    info = _case(eng, oracle, wl, 300, "five codes in the cherry", allowed=lambda i: [0, 1, 2, 3, 4] if i == 0 else [0, 1, 2, 3])
    assert info == dict(quads=0, groups=1, triples=1)
    info = _case(eng, oracle, wl, 300, "single code", allowed=lambda i: [2] if i == 1 else [3] if i == 2 else [0, 1, 2, 3])
    assert info == dict(quads=1, groups=1, triples=0)


def test_weights_and_sum_only(eng, oracle):
    wl = _workload(_shape_edges(SHAPE_B), seed=21)
    wl.setup_engine(eng)
    codes = _qcodes(wl, 300, 5)
    eng.set_patterns_codes(codes, wl.defs)
    eng.set_site_weights(_weights(300))
    try:
        want = _oracle_ll(oracle, wl, codes)
        for groups in (ONE_GROUP, TWO_GROUPS):
            assert _compare(eng, "weights", want, groups=groups)["quads"] == 1
            q, p = _run(eng, QUAD + groups, per_site=False), _run(eng, PLAIN, per_site=False)
            assert q[3][5] & 1 and p[3][5] == 0 and _hl(q) == _hl(p) == _hl(_run(eng, PLAIN)), (q, p)
    finally:
        eng.set_site_weights(None)


def test_zero_likelihood_site_and_rate0_category(eng, oracle):
    """the mixture with a rate-0 category on an 8-leaf caterpillar whose cherry has rate 0 on both edges: where its leaves
    disagree the likelihood is exactly 0 (-inf), elsewhere the rate-0 category contributes through P = I"""
    edges = caterpillar(8)
    rates = [0.0 if child in (0, 1) else 0.1 + 0.03 * i for i, (_, child) in enumerate(edges)]
    wl = tree_workload(4, edges, rates, root="custom", seed=4411, nchar=5, rate_mixture=dict(rates=[0.0, 0.4, 1.1, 2.7], prior=[0.15, 0.4, 0.05, 0.4]))
    wl.setup_engine(eng)
    codes = _qcodes(wl, 129, 8)
    codes[1] = codes[0]
    codes[0, 2], codes[1, 2] = 0, 1
    eng.set_patterns_codes(codes, wl.defs)
    eng.set_site_weights(None)
    want = _oracle_ll(oracle, wl, codes)
    for groups in (ONE_GROUP, TWO_GROUPS, GROUP_PER_CATEGORY):
        q, p = _run(eng, QUAD + groups), _run(eng, PLAIN)
        assert _info(q[3])["quads"] == 1 and np.isneginf(p[0][2]) and np.sum(np.isneginf(p[0])) == 1
        assert np.array_equal(q[0].view(np.uint64), p[0].view(np.uint64)), groups
        keep = np.isfinite(p[0])
        assert rel_err(q[0][keep], want[keep]) <= TOL


def test_rescaled_caterpillar(eng, oracle):
    """40 leaves: SCALE ops stay where they were"""
    for groups in (ONE_GROUP, TWO_GROUPS):
        info = _case(eng, oracle, _workload(caterpillar(40), seed=40), 129, "caterpillar40", groups=groups)
        assert info["quads"] == 1 and info["triples"] == 0


def test_config3(eng, oracle):
    """the plan's unit budget (the kernel has no static LDS): a table image is 200 units of 160 B; a three-leaf table adds 19
    units for one product, a shape-A table over it 26 more for a second, a shape-B table 42 for one, taken in that order.
    One group per category: 156 KB hold all of them, 14 four-leaf tables (10 A, 4 B) and the 6 three-leaf tables that are not
    below one.  Two groups (299 units of room) and one (49): three-leaf tables fill the room first and what is left holds no
    four-leaf table, so the form is the three-leaf one with 15 and 2 tables."""
    from phyly_amd import synth
    wl = synth.Workload(3)
    wl.setup_engine(eng)
    codes = wl.simulate(300)
    eng.set_patterns_codes(codes, wl.defs)
    eng.set_site_weights(None)
    want = _oracle_ll(oracle, wl, codes)
    for groups, ngroups, resident in ((ONE_GROUP, 1, 4), (TWO_GROUPS, 2, 2), (GROUP_PER_CATEGORY, 4, 1)):
        info = _compare(eng, "config 3 S=300", want, groups=groups)
        room = (156 * 1024 // resident - 200 * 160) // 160
        triples = min(16, room // 19)
        room -= 19 * triples
        upgrades = min(10, room // 26) if triples == 16 else 0
        room -= 26 * upgrades
        pairs = min(4, room // 42) if triples == 16 else 0
        assert info == dict(quads=upgrades + pairs, groups=ngroups, triples=triples - upgrades), info
    assert info == dict(quads=14, groups=4, triples=6)


def test_stale_plan_quad_bits():
    """+ 16384, + 32768, + 1024 and the group bits toggled on a live engine: after each toggle it answers bit for bit as an
    engine created with that option and reports the same kernel, variant, form, pair products and tables"""
    from phyly_amd import engine as E
    wl = _workload(caterpillar(12), seed=41)
    codes = _qcodes(wl, 300, 3)

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
        for option in (1, QUAD, 1, QUAD + TWO_GROUPS, NEVER, TRIPLE, QUAD + GROUP_PER_CATEGORY, PLAIN, QUAD + 512, 6, QUAD + ONE_GROUP, 1):
            got, want = _run(live, option), fresh(option)
            assert got[3] == want[3], (option, got[3], want[3])
            assert np.array_equal(got[0].view(np.uint64), want[0].view(np.uint64)) and got[1:3] == want[1:3], option
            seen.add((got[3][2], got[3][5] & 1, got[3][4] & 1, (got[3][4] >> 4) & 15))
        # the default and the tile kernel without; + 1024 alone: three-leaf tables only; four-leaf in one group (also without
        # pair products, which the groups need), two, four
        assert seen == {(1, 0, 0, 0), (0, 0, 0, 0), (1, 0, 1, 1), (1, 1, 1, 1), (1, 1, 1, 2), (1, 1, 1, 4)}, seen
    finally:
        live.close()


def test_patterns_replaced_on_a_live_engine():
    """first fully observed (codes 0 .. 3 at every leaf), then with the missing code at the leaves of the lowest cherry as a
    fifth code: the four-leaf table at the bottom of the caterpillar goes and its three-leaf node becomes a table; then fully
    observed again.  Every answer equals a fresh engine's bit for bit."""
    from phyly_amd import engine as E
    wl = _workload(caterpillar(9), seed=43)
    full = _qcodes(wl, 300, 6)
    part = _qcodes(wl, 300, 7, allowed=lambda i: [0, 1, 2, 3, 4] if i < 2 else [0, 1, 2, 3])

    def fresh(codes):
        e = E.Engine(0)
        try:
            wl.setup_engine(e)
            e.set_patterns_codes(codes, wl.defs)
            return _run(e, QUAD)
        finally:
            e.close()

    live = E.Engine(0)
    try:
        wl.setup_engine(live)
        counts = []
        for codes in (full, part, full):
            live.set_patterns_codes(codes, wl.defs)
            got, want = _run(live, QUAD), fresh(codes)
            assert got[3] == want[3], (got[3], want[3])
            assert np.array_equal(got[0].view(np.uint64), want[0].view(np.uint64)) and got[1:3] == want[1:3]
            p = _run(live, PLAIN)
            assert np.array_equal(got[0].view(np.uint64), p[0].view(np.uint64)) and _hl(got) == _hl(p)
            counts.append(_info(got[3]))
        assert counts[0] == counts[2] == dict(quads=1, groups=1, triples=0), counts
        assert counts[1] == dict(quads=0, groups=1, triples=1), counts
    finally:
        live.close()
