"""GPU: the streamed-code form of the k = 4 pair-table kernel (k_ll_fused4_v4s, PLK_OPT_PAIR_TABLES = 7, PLK_INFO_LL_FORM 1)
against the 1536-site tile kernel (option 6, form 0) in one engine, toggling back and forth.

Per site the two run the same instruction sequence on the same operands, so per-site ll must be bit-for-bit equal.  The
sums differ in the order of a double-double sum only (error <= S * 2^-104 relative, far below double resolution): hi + lo
as a double within one ulp, 2.3e-16 relative.  Where S <= 2000, per-site ll is also held against the oracle (binary128) at
the tolerance of tests/test_gpu_k4_variants.py.

Shapes are the smallest at which the form can go wrong: caterpillars of 5 .. 8 taxa have 4 .. 7 staged rows (every residue
mod 4 of the last chunk of a site's packed codes); 40 taxa bring SCALE ops; nchar = 16 makes a pair byte reach 255; site
counts sit around the 64-site half and the 128-site unit; one case fills every wave of every workgroup and gives some a
second unit.
"""
import numpy as np
import pytest

from helpers import oracle_model, rel_err, tree_workload
from test_gpu_kernel_families import TOL

pytestmark = pytest.mark.gpu

ULP = 2.3e-16
STREAM, TILE = 7, 6


def caterpillar(n):
    """leaves 0 .. n-1, internal nodes n .. 2n-2 (the root): the cherry (0, 1), then one leaf per level"""
    edges = [[n, 0], [n, 1]]
    for i in range(2, n):
        edges += [[n + i - 1, n + i - 2], [n + i - 1, i]]
    return edges


def _rates(E, seed):
    return np.random.default_rng(seed).uniform(0.02, 0.4, E).tolist()


def _workload(edges, *, C=4, nchar=5, root="equilibrium", data_nodes=(), seed=1):
    gamma = dict(gamma_shape=0.7, gamma_categories=C) if C > 1 else None
    wl = tree_workload(4, edges, _rates(len(edges), seed), root=root, seed=7700 + seed, gamma=gamma, nchar=max(nchar, 5), data_nodes=data_nodes)
    if nchar == 4:                       # three observable states and the all-ones row (internal nodes without data need it)
        wl.defs, wl.nchar = np.vstack([np.eye(4)[:3], np.ones((1, 4))]), 4
    return wl


def _codes(wl, S, seed, missing=0.0):
    """uniform codes over all character definitions on the leaves and the data nodes, the missing code elsewhere; with
    nchar = 16 the first sites put the largest code on every leaf (pair byte 255)"""
    rng = np.random.default_rng([seed, S])
    miss = min(4, wl.nchar - 1)          # the all-ones definition
    codes = np.full((wl.N, S), miss, dtype=np.uint8)
    leaf = wl.indptr[1:] == wl.indptr[:-1]
    for a in range(wl.N):
        if leaf[a] or a in getattr(wl, "data_nodes", ()):
            codes[a] = rng.integers(0, wl.nchar, S)
            if missing and wl.nchar > 4:
                codes[a][rng.random(S) < missing] = miss
    if wl.nchar == 16:
        codes[leaf, : max(1, S // 8)] = 15
    return codes


def _config3():
    from phyly_amd import synth
    return synth.Workload(3)


# name -> (workload factory, site counts, weights?, form expected under option 7, compare with the oracle)
CASES = {
    "rows4-cat5": (lambda: _workload(caterpillar(5), seed=5), (1, 129), False, 1),
    "rows5-cat6": (lambda: _workload(caterpillar(6), seed=6), (1, 129), False, 1),
    "rows6-cat7": (lambda: _workload(caterpillar(7), seed=7), (1, 129), False, 1),
    "rows7-cat8-sites": (lambda: _workload(caterpillar(8), seed=8), (1, 64, 65, 127, 128, 129, 1537), False, 1),
    "rescaling-cat40": (lambda: _workload(caterpillar(40), seed=40), (129,), False, 1),
    "config3-tree": (_config3, (1601,), False, 1),
    "nchar4": (lambda: _workload(caterpillar(8), nchar=4, seed=14), (129,), False, 1),
    "nchar5-missing": (lambda: _workload(caterpillar(8), nchar=5, seed=15), (129,), False, 1),
    "nchar16-byte255": (lambda: _workload(caterpillar(8), nchar=16, seed=16), (129,), False, 1),
    "internal-data": (lambda: _workload(caterpillar(8), data_nodes=(10, 12), seed=17), (129,), False, 1),
    "root-none": (lambda: _workload(caterpillar(7), root="none", seed=18), (129,), False, 1),
    "root-uniform": (lambda: _workload(caterpillar(7), root="uniform", seed=19), (129,), False, 1),
    "root-custom": (lambda: _workload(caterpillar(7), root="custom", seed=20), (129,), False, 1),
    "weights-with-zeros": (lambda: _workload(caterpillar(8), seed=21), (300,), True, 1),
    "C1": (lambda: _workload(caterpillar(8), C=1, seed=22), (129,), False, 1),
    "C2": (lambda: _workload(caterpillar(8), C=2, seed=23), (129,), False, 1),
    # 16 cherries x 16 x 16 codes x 32 B = 128 KB of tables per category: two categories do not fit the LDS
    "fallback-lds": (lambda: _workload(_balanced32(), C=2, nchar=16, seed=24), (129,), False, 0),
}


def _balanced32():
    from phyly_amd import synth
    return synth.make_tree(32, "balanced", 1)


@pytest.fixture(scope="module")
def eng():
    from phyly_amd import engine as E
    e = E.Engine(0)
    yield e
    e.set_option(E.OPT_PAIR_TABLES, 1)
    e.close()


def _ll(eng, option, form):
    from phyly_amd import engine as E
    eng.set_option(E.OPT_PAIR_TABLES, option)
    site, (hi, lo) = eng.ll()
    assert eng.info(E.INFO_LL_KERNEL) == 1 and eng.info(E.INFO_LL_VARIANT) == 6
    assert eng.info(E.INFO_LL_FORM) == form, (option, eng.info(E.INFO_LL_FORM))
    return site.copy(), hi + lo


def _weights(S):
    w = np.random.default_rng(S).uniform(0.25, 4.0, S)
    w[::7] = 0.0
    return w


def _both_forms(eng, form, tag):
    """stream, tile, stream again, tile again: equal site for site, sums within one ulp"""
    s1, t1 = _ll(eng, STREAM, form)
    s2, t2 = _ll(eng, TILE, 0)
    s3, t3 = _ll(eng, STREAM, form)
    s4, t4 = _ll(eng, TILE, 0)
    assert np.all(np.isfinite(s2)), tag
    assert np.array_equal(s1, s2) and np.array_equal(s3, s2) and np.array_equal(s4, s2), tag
    assert t3 == t1 and t4 == t2, tag                      # each form reproduces its own sum exactly
    print("%s: sum stream %.17g tile %.17g rel %.3g" % (tag, t1, t2, abs(t1 - t2) / abs(t2)))
    assert abs(t1 - t2) <= ULP * abs(t2), tag
    return s1, t1


@pytest.mark.parametrize("case", list(CASES))
def test_stream_equals_tile(eng, oracle, case):
    make, sizes, weighted, form = CASES[case]
    wl = make()
    wl.setup_engine(eng)
    m = w = None
    for S in sizes:
        codes = _codes(wl, S, seed=len(case), missing=0.2 if case == "nchar5-missing" else 0.0)
        if case == "nchar16-byte255":
            assert np.sum((codes[0] == 15) & (codes[1] == 15)) >= 1
        eng.set_patterns_codes(codes, wl.defs)
        eng.set_site_weights(_weights(S) if weighted else None)
        site, _ = _both_forms(eng, form, "%s S=%d" % (case, S))
        if S <= 2000:
            if m is None:
                m, w = oracle_model(oracle, wl, codes)
            want, _ = oracle.site_ll(m, w, codes=np.ascontiguousarray(codes.T), defs=wl.defs, precise=2)
            assert rel_err(site, want) <= TOL, (case, S)
    eng.set_site_weights(None)


def test_full_machine(eng):
    """every wave of every workgroup runs a unit, some run two, and the last unit is partial (tile form as the reference)"""
    import subprocess
    import sys
    # asked in a child process: beside the engine, torch finds no device in this one (as tests/test_gpu_query_variants.py)
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-400:]
    cus = int(r.stdout.decode().split()[-1])
    S = cus * 12 * 128 + 129
    wl = _workload(caterpillar(8), seed=8)
    wl.setup_engine(eng)
    eng.set_patterns_codes(_codes(wl, S, seed=99), wl.defs)
    eng.set_site_weights(None)
    _both_forms(eng, 1, "full machine S=%d" % S)


def _fresh(wl, codes, option, rates=None):
    from phyly_amd import engine as E
    e = E.Engine(0)
    try:
        wl.setup_engine(e)
        if rates is not None:
            e.update_edge_rates(rates)
        e.set_patterns_codes(codes, wl.defs)
        e.set_option(E.OPT_PAIR_TABLES, option)
        site, (hi, lo) = e.ll()
        return site.copy(), hi + lo, e.info(E.INFO_LL_FORM)
    finally:
        e.close()


def test_stale_state(eng):
    """new rates, new patterns (another S, other codes), another topology on the same taxa (the row order changes) and the
    option toggled: after each, the engine that has seen it all answers exactly as a fresh one"""
    from phyly_amd import engine as E
    wl = _workload(caterpillar(8), seed=31)
    codes = _codes(wl, 300, seed=1)
    wl.setup_engine(eng)
    eng.set_patterns_codes(codes, wl.defs)
    eng.set_site_weights(None)

    def same(wl_now, codes_now, rates, what):
        for option, form in ((STREAM, 1), (TILE, 0), (STREAM, 1)):
            got, tot = _ll(eng, option, form)
            want, wtot, wform = _fresh(wl_now, codes_now, option, rates)
            assert wform == form, what
            assert np.array_equal(got, want) and tot == wtot, (what, option)

    same(wl, codes, None, "first")
    rates = wl.edge_rates_csr * np.random.default_rng(3).uniform(0.5, 2.0, wl.E)
    eng.update_edge_rates(rates)
    same(wl, codes, rates, "new edge rates")
    codes2 = _codes(wl, 129, seed=2)
    eng.set_patterns_codes(codes2, wl.defs)
    same(wl, codes2, rates, "new patterns")
    # the same 8 taxa, the caterpillar built from the other end: the cherry is (7, 6), leaves join in falling order
    relabel = {i: 7 - i for i in range(8)}
    edges2 = [[p, relabel.get(c, c)] for p, c in caterpillar(8)]
    wl2 = _workload(edges2, seed=31)
    wl2.setup_engine(eng)
    eng.set_patterns_codes(codes2, wl.defs)              # a new tree drops the patterns
    same(wl2, codes2, None, "new topology")


# (option, value) steps of test_stale_plan: every option the ll plan reads, set and set back to its default
def _plan_steps():
    from phyly_amd import engine as E
    return ((E.OPT_PAIR_TABLES, 0), (E.OPT_PAIR_TABLES, 5), (E.OPT_PAIR_TABLES, 7), (E.OPT_PAIR_TABLES, 1),
            (E.OPT_FUSED_ASM, 0), (E.OPT_FUSED_ASM, 1), (E.OPT_FUSED_NS, 2), (E.OPT_FUSED_NS, 0),
            (E.OPT_FORCE_GENERIC, 1), (E.OPT_FORCE_GENERIC, 0), (E.OPT_MFMA, 2), (E.OPT_MFMA, 1),
            (E.OPT_MFMA_NS2, 1), (E.OPT_MFMA_NS2, 0), (E.OPT_VEC_REG_STACK, 0), (E.OPT_VEC_REG_STACK, 1))


def _plan_case(name):
    """k4: a partial tile and a partial 128-site unit; k20: vector <-> matrix-core; k61: two 128-site workgroups with two
    16-site groups per wave, the second nearly empty"""
    from helpers import family_workload
    if name == "k4":
        wl = _workload(caterpillar(8), seed=41)
        return wl, _codes(wl, 300, seed=3)
    wl = family_workload(20 if name == "k20" else 61)
    return wl, wl.random_codes(200 if name == "k20" else 130, seed=5)


def _answer(e):
    from phyly_amd import engine as E
    site, (hi, lo) = e.ll()
    return site.copy(), hi, lo, (e.info(E.INFO_LL_KERNEL), e.info(E.INFO_LL_VARIANT), e.info(E.INFO_LL_FORM))


@pytest.mark.parametrize("case", ["k4", "k20", "k61"])
def test_stale_plan(case):
    """one live engine, every plan-feeding option toggled and back: after each toggle it answers bit for bit as an engine
    created with that option, and reports the same kernel, variant and form.  PLK_OPT_MFMA_NS2 and PLK_OPT_VEC_REG_STACK pick
    kernels that give the same bits and the same three info values as their alternatives, so for those two a setter that forgot
    to mark the plan stale would not be seen here: what this pins for them is that the toggle leaves the answer right."""
    from phyly_amd import engine as E
    wl, codes = _plan_case(case)

    def setup(e):
        wl.setup_engine(e)
        e.set_patterns_codes(codes, wl.defs)

    fresh = {}
    defaults = {E.OPT_PAIR_TABLES: 1, E.OPT_FUSED_ASM: 1, E.OPT_FUSED_NS: 0, E.OPT_FORCE_GENERIC: 0, E.OPT_MFMA: 1, E.OPT_MFMA_NS2: 0,
                E.OPT_VEC_REG_STACK: 1}

    def fresh_answer(state):
        key = tuple(sorted((o, v) for o, v in state.items() if v != defaults[o]))      # a new engine has the defaults
        if key not in fresh:
            e = E.Engine(0)
            try:
                setup(e)
                for opt, val in key:
                    e.set_option(opt, val)
                fresh[key] = _answer(e)
            finally:
                e.close()
        return fresh[key]

    live = E.Engine(0)
    try:
        setup(live)
        _answer(live)
        state, kernels = {}, set()
        for opt, val in _plan_steps():
            live.set_option(opt, val)
            state[opt] = val
            got, want = _answer(live), fresh_answer(state)
            assert np.all(np.isfinite(got[0])), (case, opt, val)
            assert got[3] == want[3], (case, opt, val, got[3], want[3])
            assert np.array_equal(got[0], want[0]) and got[1] == want[1] and got[2] == want[2], (case, opt, val)
            kernels.add(got[3])
        # the toggles did move the plan: a test on one kernel throughout would say nothing
        # (k4: streamed, v4 tile, assembly, C++, generic; k20: vector, matrix-core, generic; k61: matrix-core, generic)
        assert len(kernels) >= {"k4": 5, "k20": 3, "k61": 2}[case], (case, kernels)
    finally:
        live.close()
