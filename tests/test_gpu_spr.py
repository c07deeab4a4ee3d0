"""GPU: plk_spr_ll / arbplf-spr against the oracle's ll of the moved tree (tests/spr_cases.py rewrites the model document).
Bars: per site |d| <= 1e-12 max(1, |ll'|); sums within 1e-12 of the long double host sum of the reference values: the bars
of tests/test_gpu_nni.py.

Worst per-site errors observed (MI355X): see the accuracy table of DESIGN.md."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import mixsens_cases
import spr_cases as cases
from helpers import K4_MODELS, QUERY_MODEL, family_workload, query_workload
from phyly_amd import engine as E_, synth
from phyly_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLIT = 0.3
_refs = {}


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _case(oracle, key, build):
    """(md, Reference) built once per module"""
    if key not in _refs:
        md = build()
        _refs[key] = (md, cases.Reference(oracle, md))
    return _refs[key]


def _dd(sums):
    sums = np.asarray(sums)
    return np.asarray(sums[..., 0], dtype=cases.LD) + np.asarray(sums[..., 1], dtype=cases.LD)


def _check_rows(ref, user, got, sums, wt, split=SPLIT):
    """got [n][S], sums [n][2] against the oracle; user: the moves in user indices"""
    worst = 0.0
    for i, (p, e) in enumerate(user):
        want = ref.move(p, e, split)
        err = cases.site_err(got[i], want)
        worst = max(worst, err)
        assert err <= cases.SITE_TOL, (p, e, err)
        if sums is not None and np.all(np.isfinite(want)):       # a row with an impossible site has no finite sum to meet
            ws = cases.weighted_sum(want, wt)
            assert abs(_dd(sums)[i] - ws) <= cases.SUM_TOL * abs(ws), (p, e, float(_dd(sums)[i]), float(ws))
    return worst


# ---------------------------------------------------------------- the k = 4 models
@pytest.mark.parametrize("S", [1, 65, 257])
@pytest.mark.parametrize("name", list(K4_MODELS) + [QUERY_MODEL])
def test_k4_models(eng, oracle, name, S):
    md, ref = _case(oracle, (name, S), lambda: cases.workload_doc(query_workload(name), S, seed=S))
    if name == "irregular" and S == 65:
        user = cases.moves_user(md["edges"])
        assert len(user) == 444
    else:
        user = cases.sample_moves(md, 48, seed=S)
        assert len(user) == 48
    assert cases.tree_kinds(md) <= cases.tree_kinds(md, user)     # every kind of move the tree has
    if name in ("irregular", "wide"):
        assert cases.tree_kinds(md, user) == set(cases.KINDS)
    csr = cases.user_to_csr(md["edges"], user)
    C = ref.w["C"]
    wt = cases.six_decade_weights(S, 3 + S)
    for layout in ("compact", "generic", "dense"):
        mixsens_cases.setup_engine(eng, oracle, md)
        if layout == "dense":
            eng.set_patterns_dense(np.ascontiguousarray(np.transpose(ref.m.B, (1, 2, 0))))
        eng.set_option(E_.OPT_FORCE_GENERIC, 1 if layout == "generic" else 0)
        try:
            got, sums = eng.spr_ll(csr, split=SPLIT)
            k4 = layout == "compact" and C <= 4
            assert eng.info(E_.INFO_SPR_KERNEL) == (1 if k4 else 2), (name, layout)
            worst = _check_rows(ref, user, got, sums, None)
            eng.set_site_weights(wt)
            got_w, sums_w = eng.spr_ll(csr, split=SPLIT)
            assert np.array_equal(got, got_w)                   # weights touch the sums only
            _check_rows(ref, user, got_w, sums_w, wt)
            print("%s S=%d %s: %d moves, worst site error %.2e" % (name, S, layout, len(user), worst))
        finally:
            eng.set_site_weights(None)
            eng.set_option(E_.OPT_FORCE_GENERIC, 0)


# ---------------------------------------------------------------- other state counts
@pytest.mark.parametrize("k", [2, 5, 13, 27, 48])
def test_family_models(eng, oracle, k):
    md, ref = _case(oracle, ("family", k), lambda: cases.workload_doc(family_workload(k), 65, seed=k))
    user = cases.sample_moves(md, 12, seed=k)
    mixsens_cases.setup_engine(eng, oracle, md)
    wt = cases.six_decade_weights(65, k)
    eng.set_site_weights(wt)
    try:
        got, sums = eng.spr_ll(cases.user_to_csr(md["edges"], user), split=SPLIT)
    finally:
        eng.set_site_weights(None)
    assert eng.info(E_.INFO_SPR_KERNEL) == 2
    print("k=%d: %d moves, worst site error %.2e" % (k, len(user), _check_rows(ref, user, got, sums, wt)))


# ---------------------------------------------------------------- carried-over scale factors
def _ladder_moves(md, n):
    """n moves spread along the ladder; the first prunes the deepest half of it onto the first edge under the root"""
    t = cases.Tree(md["edges"])
    allmv = cases.moves_user(md["edges"])
    half = min(range(t.E), key=lambda p: abs(t.size[t.edges[p][1]] - (t.E + 1) // 2))
    first = (half, 0)
    assert first in allmv and t.size[t.edges[half][1]] >= t.E // 2 - 2
    return [first] + [allmv[i] for i in np.linspace(0, len(allmv) - 1, n - 1).astype(int)]


@pytest.mark.parametrize("k", [4, 13])
def test_ladder_of_200_leaves(eng, oracle, k):
    """edge rates near 1 and observation rows scaled by 1e-4: every site likelihood is far below 2^-1022"""
    md, ref = _case(oracle, ("ladder", k), lambda: cases.ladder_doc(200, 33, seed=40 + k, k=k, C=2, leaf_scale=1e-4))
    assert np.max(ref.current()) < -1022 * np.log(2.0) - 100
    user = _ladder_moves(md, 16)
    mixsens_cases.setup_engine(eng, oracle, md)
    got, sums = eng.spr_ll(cases.user_to_csr(md["edges"], user), split=SPLIT)
    assert eng.info(E_.INFO_SPR_KERNEL) == (1 if k == 4 else 2)
    assert np.all(np.isfinite(got))
    print("ladder k=%d: worst site error %.2e" % (k, _check_rows(ref, user, got, sums, None)))


# ---------------------------------------------------------------- extremes of the split
@pytest.mark.parametrize("split", [0.0, 1.0, 0.5])
def test_extreme_splits(eng, oracle, split):
    md, ref = _case(oracle, ("irregular", 65), lambda: cases.workload_doc(query_workload("irregular"), 65, seed=65))
    user = cases.moves_user(md["edges"])
    mixsens_cases.setup_engine(eng, oracle, md)
    cur = ref.current()
    for generic in (0, 1):
        eng.set_option(E_.OPT_FORCE_GENERIC, generic)
        try:
            got, sums = eng.spr_ll(split=split)                 # the canonical list
        finally:
            eng.set_option(E_.OPT_FORCE_GENERIC, 0)
        order = cases.csr_to_user(md["edges"], E_.spr_moves(*eng._csr))
        assert sorted(order) == user
        at = {mv: i for i, mv in enumerate(order)}
        rows = [at[mv] for mv in user]
        _check_rows(ref, user, got[rows], sums[rows], None, split)
        if split == 0.0:                                        # (I1): onto a sibling edge the current tree comes back
            sib = [i for i, (p, e) in enumerate(order) if md["edges"][p][0] == md["edges"][e][0]]
            assert len(sib) >= 20
            for i in sib:
                assert cases.site_err(got[i], cur) <= cases.SITE_TOL, order[i]


def test_zero_likelihood(eng, oracle):
    """the rate-0 edge 20 -> 21: with data of two states at its ends a site is impossible wherever the edge stays whole (as
    the target e, and under every move that leaves it alone); pruned (as p) onto a sibling edge of 20 at split 0 the state of
    21 meets that of 20 again, elsewhere the site becomes possible"""
    wl = query_workload("irregular")
    md = cases.workload_doc(wl, 8, seed=8)
    z = md["edges"].index([20, 21])
    assert md["edge_rate_coefficients"][z] == 0.0
    data = [list(row) for row in md["character_data"]]
    miss = cases.missing_code(md)[1]
    for row in data:
        row[20] = row[21] = miss
    data[0][20], data[0][21] = 0, 1
    md = dict(md, character_data=data)
    ref = cases.Reference(oracle, md)
    assert np.isneginf(ref.current()[0]) and np.all(np.isfinite(ref.current()[1:]))
    user = cases.moves_user(md["edges"])
    as_e = [mv for mv in user if mv[1] == z]
    as_p = [mv for mv in user if mv[0] == z]
    assert as_e and all(np.isneginf(ref.move(p, e, 0.0)[0]) for p, e in as_e)
    assert any(np.isneginf(ref.move(p, e, 0.0)[0]) for p, e in as_p) and any(np.isfinite(ref.move(p, e, 0.0)[0]) for p, e in as_p)
    mixsens_cases.setup_engine(eng, oracle, md)
    csr = cases.user_to_csr(md["edges"], user)
    for generic in (0, 1):
        eng.set_option(E_.OPT_FORCE_GENERIC, generic)
        try:
            got, sums = eng.spr_ll(csr, split=0.0)
            assert eng.info(E_.INFO_SPR_KERNEL) == 1 + generic
            _check_rows(ref, user, got, None, None, 0.0)        # -inf exactly where the oracle has it
            bad = [i for i, mv in enumerate(user) if np.isneginf(ref.move(*mv, 0.0)[0])]
            assert bad and all(not np.isfinite(sums[i, 0] + sums[i, 1]) for i in bad)     # as plk_ll: likelihood 0 and weight 1
            wt = np.linspace(0.5, 2.0, 8)
            wt[0] = 0.0                                         # weight exactly 0: the site adds nothing
            eng.set_site_weights(wt)
            _, sums = eng.spr_ll(csr, split=0.0)
            for i, mv in enumerate(user):
                ws = cases.weighted_sum(ref.move(*mv, 0.0), wt)
                assert abs(_dd(sums)[i] - ws) <= cases.SUM_TOL * abs(ws), mv
        finally:
            eng.set_site_weights(None)
            eng.set_option(E_.OPT_FORCE_GENERIC, 0)


# ---------------------------------------------------------------- chunking, order, repetition, long lists
def _full(eng, oracle, name, S):
    md, ref = _case(oracle, (name, S), lambda: cases.workload_doc(query_workload(name), S, seed=S))
    mixsens_cases.setup_engine(eng, oracle, md)
    return md


def test_chunked_call_gives_the_same_bits(eng, oracle):
    for name in ("irregular", "balanced64"):                    # the k = 4 kernel and the generic one
        _full(eng, oracle, name, 257)
        moves = E_.spr_moves(*eng._csr)[::7]
        wt = cases.six_decade_weights(257, 9)
        eng.set_site_weights(wt)
        try:
            whole, whole_sums = eng.spr_ll(moves, split=SPLIT)
            eng.set_option(E_.OPT_SITE_CHUNK, 100)
            parts, part_sums = eng.spr_ll(moves, split=SPLIT)
        finally:
            eng.set_option(E_.OPT_SITE_CHUNK, 0)
            eng.set_site_weights(None)
        assert np.array_equal(whole, parts)
        # the sums of three chunks are added in another order: same values to the sums bar
        assert np.all(np.abs(_dd(whole_sums) - _dd(part_sums)) <= cases.SUM_TOL * np.abs(_dd(whole_sums)))


def test_order_and_repetition(eng, oracle):
    for name in ("balanced32", "irregular", "balanced64"):
        _full(eng, oracle, name, 65)
        canon = E_.spr_moves(*eng._csr)
        n = len(canon)
        base, base_sums = eng.spr_ll(split=SPLIT)
        assert base.shape == (n, 65)
        rng = np.random.default_rng(5)
        pick = np.concatenate([rng.permutation(n)[: n // 2], [3, 3, 0]])      # half of the list, shuffled, repeats
        got, sums = eng.spr_ll(canon[pick], split=SPLIT)
        assert np.array_equal(got, base[pick]) and np.array_equal(sums, base_sums[pick])
        one, one_sum = eng.spr_ll(canon[[n // 3]], split=SPLIT)  # one move alone
        assert np.array_equal(one[0], base[n // 3]) and np.array_equal(one_sum[0], base_sums[n // 3])


def test_600_moves_of_one_prune_edge_run_in_three_passes(eng, oracle):
    """the later passes of a prune edge read the stored vectors of the pruned tree"""
    for k in (4, 13):
        md, ref = _case(oracle, ("ladder9", k), lambda: cases.ladder_doc(200, 9, seed=50 + k, k=k, C=2))
        mixsens_cases.setup_engine(eng, oracle, md)
        canon = E_.spr_moves(*eng._csr)
        count = np.bincount(canon[:, 0])
        p = int(len(count) - 1 - np.argmax(count[::-1]))        # the last of the prune edges with the most targets: a deep leaf
        mine = canon[canon[:, 0] == p]
        assert len(mine) > 256
        base, base_sums = eng.spr_ll(mine, split=SPLIT)
        pick = (np.arange(600) * 7) % len(mine)
        got, sums = eng.spr_ll(mine[pick], split=SPLIT)
        assert got.shape == (600, 9)
        assert np.array_equal(got, base[pick]) and np.array_equal(sums, base_sums[pick])
        few = [0, 255, 256, 511, 512, 599]
        user = cases.csr_to_user(md["edges"], mine[pick][few])
        _check_rows(ref, user, got[few], sums[few], None)


# ---------------------------------------------------------------- against the engine itself
def test_against_ll_of_a_fresh_engine_on_the_moved_tree(eng):
    wl = query_workload("irregular")
    S = 100003
    codes = np.ascontiguousarray(np.tile(wl.random_codes(257, seed=3), (1, S // 257 + 1))[:, :S])
    wl.setup_engine(eng)
    eng.set_patterns_codes(codes, wl.defs)
    t = cases.Tree(wl.edges)
    allmv = cases.moves_user(wl.edges)
    user = [next(mv for mv in allmv if t.edges[mv[0]][1] in t.kids and t.edges[mv[1]][1] == t.edges[mv[0]][0]),      # an inner subtree onto the edge into w
            next(mv for mv in allmv if t.edges[mv[0]][1] not in t.kids and not t.is_below(t.edges[mv[0]][0], t.edges[mv[1]][0])
                 and not t.is_below(t.edges[mv[1]][0], t.edges[mv[0]][0])),                                          # a leaf into a far subtree
            next(mv for mv in allmv if t.edges[mv[0]][0] == t.edges[mv[1]][0])]                                      # onto a sibling edge
    got, sums = eng.spr_ll(cases.user_to_csr(wl.edges, user), split=SPLIT)
    assert eng.info(E_.INFO_SPR_KERNEL) == 1
    k0 = wl.prepare()
    mode, rw = wl.root_engine()
    miss = next(c for c in range(wl.nchar) if np.all(wl.defs[c] == 1.0))
    for i, (p, e) in enumerate(user):
        u, b = wl.edges[e]
        edges2 = [list(x) for x in wl.edges]
        edges2[e] = [u, wl.N]
        edges2[p] = [wl.N, wl.edges[p][1]]
        edges2 += [[wl.N, b]]
        rates2 = list(wl.edge_rates) + [(1.0 - SPLIT) * wl.edge_rates[e]]
        rates2[e] = SPLIT * wl.edge_rates[e]
        indptr, indices, preorder, order2 = synth.csr_from_edges(edges2)
        rates = np.zeros(len(edges2))
        rates[order2] = rates2
        codes2 = np.ascontiguousarray(np.vstack([codes, np.full((1, S), miss, dtype=codes.dtype)]))
        fresh = Engine(0)
        try:
            fresh.set_tree(indptr, indices, preorder)
            fresh.set_model(k0["Qn"], rates, k0["cat_rates"], k0["cat_prior"], mode, rw, Qn_lo=k0["Qn_lo"])
            fresh.set_patterns_codes(codes2, wl.defs)
            want, (hi, lo) = fresh.ll()
        finally:
            fresh.close()
        assert cases.site_err(got[i], want) <= cases.SITE_TOL, (p, e)
        assert abs(float(_dd(sums)[i]) - (hi + lo)) <= cases.SUM_TOL * abs(hi + lo)


# ---------------------------------------------------------------- refusals
def test_refusals(eng, oracle):
    md = _full(eng, oracle, "irregular", 65)
    canon = E_.spr_moves(*eng._csr)
    E = len(md["edges"])
    good = canon[::9]
    base, base_sums = eng.spr_ll(good, split=SPLIT)
    p, e = map(int, good[5])
    # a target below the pruned edge: an inner subtree and the first edge inside it
    t = cases.Tree(md["edges"])
    inner_user = next(a for a in range(E) if t.edges[a][1] in t.kids)
    under_user = next(b for b in range(E) if t.edges[b][0] == t.edges[inner_user][1])
    (inner, under), = cases.user_to_csr(md["edges"], [(inner_user, under_user)]).tolist()
    for moves, split, word in (([[p, e], [E, e]], SPLIT, "pair 1 (%d, %d)" % (E, e)), ([[p, -1]], SPLIT, "pair 0 (%d, -1)" % p),
                               ([[p, e], [p, e], [p, p]], SPLIT, "pair 2 (%d, %d)" % (p, p)),
                               ([[inner, under]], SPLIT, "pair 0 (%d, %d)" % (inner, under)),
                               (good, -0.1, "split"), (good, 1.5, "split"), (good, np.nan, "split"), (good, np.inf, "split")):
        with pytest.raises(EngineError) as ei:
            eng.spr_ll(moves, split=split)
        assert ei.value.code == E_.E_ARG and word in str(ei.value), (word, str(ei.value))
    with pytest.raises(EngineError) as ei:
        eng.spr_ll([[inner, under]], split=SPLIT)
    assert "below" in str(ei.value)
    with pytest.raises(EngineError) as ei:
        eng._check(eng._lib.plk_spr_ll(eng._h, 7, None, 0.5, None, None))       # NULL = the canonical list: its length
    assert "canonical list" in str(ei.value)
    none, no_sums = eng.spr_ll(good, split=SPLIT, per_site=False, want_sums=False)       # nothing asked for: checked, nothing runs
    assert none is None and no_sums is None
    with pytest.raises(EngineError):
        eng.spr_ll(good, split=2.0, per_site=False, want_sums=False)
    again, again_sums = eng.spr_ll(good, split=SPLIT)           # the engine stays usable and gives the same bits
    assert np.array_equal(base, again) and np.array_equal(base_sums, again_sums)
    fresh = Engine(0)                                           # nothing set yet
    try:
        with pytest.raises(EngineError) as ei:
            fresh.spr_ll(good, split=SPLIT)
        assert ei.value.code == E_.E_ARG and "must be set" in str(ei.value)
    finally:
        fresh.close()


# ---------------------------------------------------------------- history
def _history_steps(Q, moves, new_rates, old_rates, order):
    def flat(*xs):
        return tuple(np.asarray(x) for x in xs if x is not None)
    spr = ("spr", lambda e: flat(*e.spr_ll(moves, split=SPLIT)))
    steps = {"ll": ("ll", lambda e: flat(e.ll()[0], e.ll()[1])), "deriv": ("deriv", lambda e: flat(*e.deriv())),
             "nni": ("nni", lambda e: flat(*e.nni_ll())),
             "place": ("place", lambda e: flat(*e.place_ll(q_codes=Q, split=SPLIT, pendant_rate=0.07))),
             "rates": ("update_edge_rates", lambda e: (e.update_edge_rates(new_rates), ())[1]),
             "back": ("update_edge_rates_back", lambda e: (e.update_edge_rates(old_rates), ())[1])}
    out = []
    for name in order:
        out += [steps[name], spr]
    return [spr] + out


@pytest.mark.parametrize("order", [("ll", "deriv", "nni", "place", "rates", "back"), ("nni", "rates", "ll", "place", "back", "deriv"),
                                   ("rates", "place", "deriv", "back", "nni", "ll")], ids=["a", "b", "c"])
def test_history(order):
    """the scan between ll, deriv, nni_ll, place_ll and a rate change and back on one engine: every result bit for bit what
    a fresh engine brought to the same state gives, and what a run without the scan gives"""
    wl = query_workload("balanced32")
    S = 300
    codes = wl.random_codes(S, seed=2)
    rng = np.random.default_rng(6)
    Q = rng.integers(0, wl.nchar, (2, S)).astype(np.uint8)
    old_rates = np.asarray(wl.edge_rates_csr, dtype=float)
    new_rates = old_rates * np.linspace(0.7, 1.4, wl.E)
    indptr, indices = synth.csr_from_edges(wl.edges)[:2]
    moves = E_.spr_moves(indptr, indices)[::41]
    steps = _history_steps(Q, moves, new_rates, old_rates, order)
    wt = cases.six_decade_weights(S, 21)

    def fresh(updated):
        e = Engine(0)
        wl.setup_engine(e)
        e.set_patterns_codes(codes, wl.defs)
        e.set_site_weights(wt)
        if updated:
            e.update_edge_rates(new_rates)
        return e

    one = fresh(False)
    try:
        seq = [call(one) for _, call in steps]
    finally:
        one.close()
    two = fresh(False)                                          # the same queries without the scan
    try:
        bare = {i: call(two) for i, (name, call) in enumerate(steps) if name != "spr"}
    finally:
        two.close()
    updated = False
    for i, (name, call) in enumerate(steps):
        if name.startswith("update_edge_rates"):
            updated = name == "update_edge_rates"
            continue
        e = fresh(updated)
        try:
            alone = call(e)
        finally:
            e.close()
        assert len(alone) == len(seq[i]) > 0
        for x, y in zip(alone, seq[i]):
            assert np.array_equal(x, y, equal_nan=True), (i, name)
        if name != "spr":
            for x, y in zip(bare[i], seq[i]):
                assert np.array_equal(x, y, equal_nan=True), (i, name)


# ---------------------------------------------------------------- groups
def test_group_of_two_engines(oracle):
    md, ref = _case(oracle, ("irregular", 257), lambda: cases.workload_doc(query_workload("irregular"), 257, seed=257))
    m = oracle.parse_model(md)
    k0 = mixsens_cases.product_k0(m)
    codes = np.ascontiguousarray(np.asarray(md["character_data"]).astype(np.uint8).T)
    defs = np.asarray(md["character_definitions"], dtype=float)
    rw = np.asarray(m.root_custom, dtype=float)
    wt = cases.six_decade_weights(257, 5)
    moves = np.ascontiguousarray(E_.spr_moves(m.indptr, m.indices)[::5])
    n = len(moves)
    lib = E_.load_library()
    vp, ci, cl, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_double
    lib.plk_group_create.argtypes = [ctypes.POINTER(vp), ci, vp]
    lib.plk_group_destroy.argtypes = [vp]
    lib.plk_group_set_tree.argtypes = [vp, ci, vp, vp, vp]
    lib.plk_group_set_model.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp, ci, vp]
    lib.plk_group_set_patterns_codes.argtypes = [vp, cl, vp, ci, vp]
    lib.plk_group_set_site_weights.argtypes = [vp, vp]
    lib.plk_group_spr_ll.argtypes = [vp, ci, vp, cd, vp, vp]
    lib.plk_group_last_error.argtypes = [vp]
    lib.plk_group_last_error.restype = ctypes.c_char_p
    results = []
    for devs in ([0], [0, 0]):
        g = vp()
        dev = np.array(devs, dtype=np.int32)
        assert lib.plk_group_create(ctypes.byref(g), len(devs), E_._ptr(dev)) == 0
        try:
            def ok(rc):
                assert rc == 0, lib.plk_group_last_error(g)
            ok(lib.plk_group_set_tree(g, m.N, E_._ptr(m.indptr), E_._ptr(m.indices), E_._ptr(m.preorder)))
            er = np.ascontiguousarray(m.edge_rates_csr, dtype=float)
            ok(lib.plk_group_set_model(g, m.k, k0["C"], E_._ptr(k0["Qn"]), E_._ptr(k0["Qn_lo"]), E_._ptr(er), E_._ptr(k0["cat_rates"]),
                                       E_._ptr(k0["cat_prior"]), m.root_mode, E_._ptr(rw)))
            ok(lib.plk_group_set_patterns_codes(g, 257, E_._ptr(codes), len(defs), E_._ptr(defs)))
            ok(lib.plk_group_set_site_weights(g, E_._ptr(wt)))
            out, sums = np.zeros((n, 257)), np.zeros((n, 2))
            ok(lib.plk_group_spr_ll(g, n, E_._ptr(moves), SPLIT, E_._ptr(out), E_._ptr(sums)))
            results.append((out, sums))
        finally:
            lib.plk_group_destroy(g)
    (one, one_sums), (two, two_sums) = results
    assert np.array_equal(one, two)
    assert np.all(np.abs(_dd(one_sums) - _dd(two_sums)) <= cases.SUM_TOL * np.abs(_dd(one_sums)))
    user = cases.csr_to_user(md["edges"], moves[:6])
    _check_rows(ref, user, one[:6], one_sums[:6], wt)


# ---------------------------------------------------------------- JSON, CLI, Python
FELSENSTEIN = os.path.join(ROOT, "tests", "golden", "examples", "Felsenstein.2004.fig.16.4", "ll", "in.json")


def _cli(doc, env=None):
    p = subprocess.run([os.path.join(ROOT, "phyly_amd", "csrc", "arbplf-spr")], input=json.dumps(doc).encode(),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **(env or {})))
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def _three_ways(doc):
    import arbplf
    from phyly_amd import arbplf as string_api
    texts = [arbplf.arbplf_spr(json.dumps(doc)), string_api._call("arbplf_spr", json.dumps(doc))]
    rc, text, err = _cli(doc)
    assert rc == 0, err
    texts.append(text.strip())
    assert texts[0] == texts[1] == texts[2]                     # byte for byte
    return json.loads(texts[0])


def _felsenstein():
    with open(FELSENSTEIN) as f:
        base = json.load(f)
    md = base["model_and_data"]
    assert len(md["probability_array"]) == 1 and len(md["edges"]) == 7
    rows = [md["probability_array"][0]]
    for s in range(1, 5):                                       # more sites: the document's site with the leaf states rotated
        rows.append([row[s % 4:] + row[:s % 4] for row in rows[0]])
    return {"model_and_data": dict(md, probability_array=rows)}


@pytest.mark.parametrize("reduction", [None, {"aggregation": "sum"}, {"selection": [3, 0, 3], "aggregation": [0.5, -2.0, 1.25]}], ids=["sites", "sum", "weighted"])
@pytest.mark.parametrize("listed", [False, True])
def test_json_cli_python(oracle, reduction, listed):
    base = _felsenstein()
    md = base["model_and_data"]
    S = len(md["probability_array"])
    allmv = cases.moves_user(md["edges"])
    moves = [allmv[11], allmv[2], allmv[-1], allmv[11]] if listed else allmv      # not in canonical order, with a repeat
    doc = dict(base, spr={"split": 0.25})
    if listed:
        doc["spr"]["moves"] = [list(mv) for mv in moves]
    if reduction:
        doc["site_reduction"] = reduction
    out = _three_ways(doc)
    ref = cases.Reference(oracle, md)
    want = {mv: ref.move(*mv, 0.25) for mv in set(moves)}
    rows = out["data"]
    if reduction is None:
        assert out["columns"] == ["site", "prune", "target", "value"]
        assert [r[:3] for r in rows] == [[s, p, e] for s in range(S) for p, e in moves]
        for s, p, e, v in rows:
            assert abs(v - want[p, e][s]) <= cases.SITE_TOL * max(1.0, abs(v))
    else:
        assert out["columns"] == ["prune", "target", "value"]
        assert [r[:2] for r in rows] == [list(mv) for mv in moves]
        sel = reduction.get("selection", list(range(S)))
        wts = reduction["aggregation"] if isinstance(reduction["aggregation"], list) else [1.0] * len(sel)
        for p, e, v in rows:
            ws = float(sum(cases.LD(w) * cases.LD(want[p, e][s]) for w, s in zip(wts, sel)))
            assert abs(v - ws) <= cases.SUM_TOL * max(1.0, abs(ws))


def test_json_defaults(oracle):
    """without "spr": every move at split 0.5"""
    base = _felsenstein()
    md = base["model_and_data"]
    out = _three_ways(dict(base, site_reduction={"aggregation": "sum"}))
    allmv = cases.moves_user(md["edges"])
    assert [tuple(r[:2]) for r in out["data"]] == allmv
    ref = cases.Reference(oracle, md)
    for p, e, v in out["data"][::5]:
        ws = float(np.sum(np.asarray(ref.move(p, e, 0.5), dtype=cases.LD)))
        assert abs(v - ws) <= cases.SUM_TOL * abs(ws)


def test_json_on_a_compressed_alignment(oracle):
    """40 sites of three patterns: duplicate columns are computed once and every site gets its pattern's value"""
    md1 = mixsens_cases.five_taxon_doc(3, 4, seed=9)
    which = [s % 3 for s in range(40)]
    md = dict(md1, character_data=[md1["character_data"][w] for w in which])
    moves = cases.sample_moves(md, 9, seed=2)
    ref = cases.Reference(oracle, md)
    out = _three_ways({"model_and_data": md, "spr": {"moves": [list(mv) for mv in moves], "split": 0.4}})
    got = {(s, p, e): v for s, p, e, v in out["data"]}
    assert len(got) == 40 * len(set(moves))
    for (s, p, e), v in got.items():
        assert abs(v - ref.move(p, e, 0.4)[s]) <= cases.SITE_TOL * max(1.0, abs(v))
        assert v == got[s % 3, p, e]
    summed = _three_ways({"model_and_data": md, "spr": {"moves": [list(mv) for mv in moves], "split": 0.4}, "site_reduction": {"aggregation": "sum"}})
    for p, e, v in summed["data"]:
        ws = float(np.sum(np.asarray(ref.move(p, e, 0.4), dtype=cases.LD)))
        assert abs(v - ws) <= cases.SUM_TOL * abs(ws)


def test_json_errors():
    import arbplf
    base = _felsenstein()
    for spr, word in (({"moves": [[0, 0]]}, "no move"), ({"moves": [[0, 7]]}, "out of range"), ({"moves": [[0.5, 1]]}, "integers"),
                      ({"moves": [[0, 1, 2]]}, "pair"), ({"moves": 3}, "moves"), ({"split": 1.5}, "split"), ({"split": "half"}, "split"),
                      ({"swaps": []}, "swaps"), ([1], "spr")):
        doc = dict(base, spr=spr)
        with pytest.raises(RuntimeError):
            arbplf.arbplf_spr(json.dumps(doc))
        rc, text, err = _cli(doc)
        assert rc != 0 and text == "" and word in err, (spr, err)
    t = cases.Tree(base["model_and_data"]["edges"])
    inner = next(a for a in range(t.E) if t.edges[a][1] in t.kids)
    under = next(b for b in range(t.E) if t.edges[b][0] == t.edges[inner][1])
    rc, text, err = _cli(dict(base, spr={"moves": [[inner, under]]}))
    assert rc != 0 and text == "" and "no move" in err


def test_cli_without_a_gpu_has_no_fallback():
    rc, text, err = _cli(dict(_felsenstein(), spr={}), env={"HIP_VISIBLE_DEVICES": "", "ROCR_VISIBLE_DEVICES": ""})
    assert rc == 255 and text == "" and "no CPU fallback" in err
