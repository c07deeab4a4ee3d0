#!/usr/bin/env python3
"""What plk_spr_ll is worth against the loop a caller had to write before it:
  python tools/time_spr.py --config 3 --sites 2000000 [--out profiles/spr_cfg3.json]
  (a) plk_spr_ll over the canonical list of the tree (every prune edge onto every edge outside its subtree), sums only:
      wall clock and PLK_INFO_LAST_QUERY_NS;
  (b) the loop the call replaces, on --loop-moves moves spread evenly over the list: per move the moved tree (one node and
      one edge more), plk_set_tree, plk_set_model, plk_set_patterns_codes with a missing-code row for the new node
      appended, plk_ll sums only; wall clock per move with and without the pattern upload.  Putting the new node's row
      under the tree's code bytes on the host ("augment") is timed on its own and belongs to neither figure.  The whole
      list is NOT run: its time is the per-move time multiplied by the number of moves, and the output marks it as
      extrapolated;
  (c) one plk_deriv, sums only, for scale.
One process, medians of --reps repetitions after one untimed run of each.  Before anything is timed the sums of the moves of
(b) must agree with those of (a) to 1e-12 relative, the bar the tests hold plk_ll sums to; the tool fails otherwise.  Prints
one JSON line; the kernels' register counts come from the build's saved assembly when it is there."""
import argparse
import datetime
import glob
import json
import os
import re
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from phyly_amd import synth, engine as E   # noqa: E402

SUM_TOL = 1e-12
SPLIT = 0.5


def register_counts():
    out = {}
    for path in glob.glob(os.path.join(ROOT, "phyly_amd", "csrc", "build", "plk_engine-hip-amdgcn-*.s")):
        text = open(path).read()
        for blk in text.split("  - .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            if "spr" in name:
                g = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
                out[name] = dict(agpr=int(blk.split("\n")[0]), vgpr=g("vgpr_count"), sgpr=g("sgpr_count"),
                                 scratch_bytes=g("private_segment_fixed_size"), vgpr_spills=g("vgpr_spill_count"))
    return out


def moved_tree(wl, csr_p, csr_e):
    """(indptr, indices, preorder, rates in CSR order) of the tree with CSR edge csr_p pruned and attached to CSR edge csr_e"""
    order = np.asarray(wl.order)
    p, e = int(np.flatnonzero(order == csr_p)[0]), int(np.flatnonzero(order == csr_e)[0])
    u, b = wl.edges[e]
    edges = [list(x) for x in wl.edges]
    edges[e] = [u, wl.N]
    edges[p] = [wl.N, wl.edges[p][1]]
    edges += [[wl.N, b]]
    r = wl.edge_rates[e]
    rates_user = list(wl.edge_rates) + [(1.0 - SPLIT) * r]
    rates_user[e] = SPLIT * r
    indptr, indices, preorder, order2 = synth.csr_from_edges(edges)
    rates = np.zeros(len(edges))
    rates[order2] = rates_user
    return indptr, indices, preorder, rates


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=3)
    ap.add_argument("--sites", type=int, default=2_000_000)
    ap.add_argument("--loop-moves", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    wl = synth.Workload(a.config)
    S = a.sites
    eng = E.Engine(0)
    wl.setup_engine(eng)
    codes = wl.simulate(S)
    eng.set_patterns_codes(codes, wl.defs)
    miss = next(c for c in range(wl.nchar) if np.all(np.asarray(wl.defs)[c] == 1.0))
    moves = E.spr_moves(wl.indptr, wl.indices)
    nmoves = len(moves)
    loop_moves = [int(t) for t in np.linspace(0, nmoves - 1, a.loop_moves).astype(int)]
    trees = {t: moved_tree(wl, *map(int, moves[t])) for t in loop_moves}
    k0 = wl.prepare()
    res = {}

    def set_model(rates):
        eng.set_model(k0["Qn"], rates, k0["cat_rates"], k0["cat_prior"], E.ROOT_EQUILIBRIUM, k0["pi"], Qn_lo=k0["Qn_lo"])

    def scan():
        res["a"] = eng.spr_ll(split=SPLIT, per_site=False)[1]

    def rebuild_loop():
        sums = np.zeros((len(loop_moves), 2))
        part = dict(augment=0.0, set_tree=0.0, set_model=0.0, set_patterns=0.0, ll=0.0)
        clock = time.perf_counter
        for i, t in enumerate(loop_moves):
            t0 = clock()
            codes2 = np.concatenate([codes, np.full((1, S), miss, dtype=codes.dtype)])
            indptr, indices, preorder, rates = trees[t]
            t1 = clock()
            eng.set_tree(indptr, indices, preorder)
            t2 = clock()
            set_model(rates)
            t3 = clock()
            eng.set_patterns_codes(codes2, wl.defs)
            t4 = clock()
            sums[i] = eng.ll(per_site=False)[1]
            t5 = clock()
            for key, dt in zip(part, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4)):
                part[key] += dt * 1e3
        res["b"] = sums
        res["b_parts"] = part

    def current_tree():
        eng.set_tree(wl.indptr, wl.indices, wl.preorder)
        set_model(wl.edge_rates_csr)
        eng.set_patterns_codes(codes, wl.defs)

    # agreement first (these are the untimed runs as well)
    scan()
    spr_kernel, down4 = eng.info(E.INFO_SPR_KERNEL), eng.info(E.INFO_DOWN4_KERNEL)
    rebuild_loop()
    current_tree()
    sa = res["a"][loop_moves]
    sa = sa[:, 0].astype(np.longdouble) + sa[:, 1]
    sb = res["b"][:, 0].astype(np.longdouble) + res["b"][:, 1]
    diff = float(np.max(np.abs(sa - sb) / np.abs(sb)))
    if not diff <= SUM_TOL:
        raise SystemExit("time_spr: the sums of plk_spr_ll and of the rebuild loop differ by %.3e relative (bar %.0e)" % (diff, SUM_TOL))

    wall_a, dev_a, wall_b, parts_b = [], [], [], []
    for _ in range(a.reps):                 # alternating, so that drift of the machine hits both alike
        t0 = time.perf_counter()
        scan()
        wall_a.append((time.perf_counter() - t0) * 1e3)
        dev_a.append(eng.info(E.INFO_QUERY_NS) * 1e-6)
        t0 = time.perf_counter()
        rebuild_loop()
        wall_b.append((time.perf_counter() - t0) * 1e3)
        parts_b.append(res["b_parts"])
        current_tree()
    eng.deriv(per_site=False)
    wall_c, dev_c = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        eng.deriv(per_site=False)
        wall_c.append((time.perf_counter() - t0) * 1e3)
        dev_c.append(eng.info(E.INFO_QUERY_NS) * 1e-6)
    med = statistics.median
    nb = len(loop_moves)
    b_move = med([w - p["augment"] for w, p in zip(wall_b, parts_b)]) / nb
    b_move_no_upload = med([w - p["set_patterns"] - p["augment"] for w, p in zip(wall_b, parts_b)]) / nb
    a_move = med(wall_a) / nmoves
    out = {"date": datetime.date.today().isoformat(), "box": "one MI355X (gfx950)", "config": a.config, "name": wl.name, "sites": S,
           "states": wl.k, "categories": eng.C, "edges": eng.E, "moves": nmoves, "prune_edges": int(len(set(moves[:, 0].tolist()))), "split": SPLIT,
           "timing": "one process, medians of %d repetitions after one untimed run of each, (a) and (b) alternating; sums only, "
                     "no per-site output; wall = host clock around synchronous calls, device = PLK_INFO_LAST_QUERY_NS" % a.reps,
           "spr_kernel": spr_kernel, "down4_kernel": down4,
           "a_spr_ll_wall_ms": med(wall_a), "a_spr_ll_device_ms": med(dev_a), "a_per_move_wall_ms": a_move,
           "b_loop_moves": nb, "b_loop_wall_ms": med(wall_b), "b_per_move_wall_ms": b_move,
           "b_per_move_note": "per-move figures leave out the host-side concatenation of the code rows (augment in b_wall_ms_by_call)",
           "b_per_move_without_pattern_upload_wall_ms": b_move_no_upload,
           "b_wall_ms_by_call": {key: med([p[key] for p in parts_b]) for key in parts_b[0]},
           "b_all_moves_wall_ms_extrapolated": b_move * nmoves,
           "b_all_moves_without_pattern_upload_wall_ms_extrapolated": b_move_no_upload * nmoves,
           "extrapolated": "the two *_extrapolated figures are per-move times of %d measured moves multiplied by %d moves; the loop was not run on all of them" % (nb, nmoves),
           "a_per_move_below_b_per_move_without_pattern_upload": bool(a_move < b_move_no_upload),
           "b_over_a_per_move": b_move / a_move, "b_without_pattern_upload_over_a_per_move": b_move_no_upload / a_move,
           "c_deriv_wall_ms": med(wall_c), "c_deriv_device_ms": med(dev_c), "a_over_c_device": med(dev_a) / med(dev_c),
           "a_vs_b_max_rel_diff_of_sums": diff,
           "all_wall_ms": {"a": wall_a, "b": wall_b, "c": wall_c}, "registers": register_counts()}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
