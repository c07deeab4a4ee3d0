#!/usr/bin/env python3
"""What plk_nni_ll is worth against the loop a caller had to write before it:
  python tools/time_nni.py --config 3 --sites 2000000 [--out profiles/nni_cfg3.json]
  (a) plk_nni_ll on the canonical list of swaps, sums only: wall clock and PLK_INFO_LAST_QUERY_NS;
  (b) per swap plk_set_tree with the swapped tree, plk_set_model with the rates in its CSR order and
      plk_set_patterns_codes again (a new tree drops the model and the patterns: plk_update_edge_rates alone is refused),
      plk_ll sums only: wall clock over the whole list (every call is synchronous, so the clock stops after the last
      device operation), and the same clock split by call, so that the share of the pattern upload is on record;
  (c) one plk_deriv, sums only, for scale.
One process, medians of --reps repetitions after one untimed run of each.  Before anything is timed the sums of (a) and
(b) must agree to 1e-12 relative, the bar the tests hold plk_ll sums to; the tool fails otherwise.  Prints one JSON line;
the kernels' register counts come from the build's saved assembly when it is there."""
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


def register_counts():
    out = {}
    for path in glob.glob(os.path.join(ROOT, "phyly_amd", "csrc", "build", "plk_engine-hip-amdgcn-*.s")):
        text = open(path).read()
        for blk in text.split("  - .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            if "nni" in name:
                g = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
                out[name] = dict(agpr=int(blk.split("\n")[0]), vgpr=g("vgpr_count"), sgpr=g("sgpr_count"),
                                 scratch_bytes=g("private_segment_fixed_size"), vgpr_spills=g("vgpr_spill_count"))
    return out


def swapped_trees(wl, swaps_csr):
    """(indptr, indices, preorder, rates in CSR order) of every swapped tree, prepared outside the clock: a caller's tree
    search holds its candidate trees in this form anyway"""
    order = np.asarray(wl.order)
    user_of = np.empty(wl.E, dtype=int)
    user_of[order] = np.arange(wl.E)
    trees = []
    for a, b in swaps_csr:
        ua, ub = user_of[a], user_of[b]
        edges = [list(e) for e in wl.edges]
        edges[ua][0], edges[ub][0] = wl.edges[ub][0], wl.edges[ua][0]
        indptr, indices, preorder, order2 = synth.csr_from_edges(edges)
        rates = np.zeros(wl.E)
        rates[order2] = wl.edge_rates
        trees.append((indptr, indices, preorder, rates))
    return trees


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=3)
    ap.add_argument("--sites", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    wl = synth.Workload(a.config)
    S = a.sites
    eng = E.Engine(0)
    wl.setup_engine(eng)
    codes = wl.simulate(S)
    eng.set_patterns_codes(codes, wl.defs)
    swaps = E.nni_swaps(wl.indptr, wl.indices)
    trees = swapped_trees(wl, swaps)
    res = {}

    k0 = wl.prepare()

    def set_model(rates):
        eng.set_model(k0["Qn"], rates, k0["cat_rates"], k0["cat_prior"], E.ROOT_EQUILIBRIUM, k0["pi"], Qn_lo=k0["Qn_lo"])

    def scan():
        res["a"] = eng.nni_ll(per_site=False)[1]

    def rebuild_loop():
        sums = np.zeros((len(trees), 2))
        part = dict(set_tree=0.0, set_model=0.0, set_patterns=0.0, ll=0.0)
        clock = time.perf_counter
        for i, (indptr, indices, preorder, rates) in enumerate(trees):
            t0 = clock()
            eng.set_tree(indptr, indices, preorder)
            t1 = clock()
            set_model(rates)
            t2 = clock()
            eng.set_patterns_codes(codes, wl.defs)
            t3 = clock()
            sums[i] = eng.ll(per_site=False)[1]
            t4 = clock()
            part["set_tree"] += (t1 - t0) * 1e3
            part["set_model"] += (t2 - t1) * 1e3
            part["set_patterns"] += (t3 - t2) * 1e3
            part["ll"] += (t4 - t3) * 1e3
        res["b"] = sums
        res["b_parts"] = part

    def current_tree():
        eng.set_tree(wl.indptr, wl.indices, wl.preorder)
        set_model(wl.edge_rates_csr)
        eng.set_patterns_codes(codes, wl.defs)

    # agreement first (these are the untimed runs as well)
    scan()
    nni_kernel, down4 = eng.info(E.INFO_NNI_KERNEL), eng.info(E.INFO_DOWN4_KERNEL)
    rebuild_loop()
    ll_kernel, ll_form = eng.info(E.INFO_LL_KERNEL), eng.info(E.INFO_LL_FORM)
    current_tree()
    sa = res["a"][:, 0].astype(np.longdouble) + res["a"][:, 1]
    sb = res["b"][:, 0].astype(np.longdouble) + res["b"][:, 1]
    diff = float(np.max(np.abs(sa - sb) / np.abs(sb)))
    if not diff <= SUM_TOL:
        raise SystemExit("time_nni: the sums of plk_nni_ll and of the rebuild loop differ by %.3e relative (bar %.0e)" % (diff, SUM_TOL))

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
    out = {"date": datetime.date.today().isoformat(), "box": "one MI355X (gfx950)", "config": a.config, "name": wl.name, "sites": S,
           "states": wl.k, "categories": eng.C, "edges": eng.E, "swaps": int(len(swaps)),
           "timing": "one process, medians of %d repetitions after one untimed run of each, (a) and (b) alternating; sums only, "
                     "no per-site output; wall = host clock around synchronous calls, device = PLK_INFO_LAST_QUERY_NS" % a.reps,
           "nni_kernel": nni_kernel, "down4_kernel": down4, "ll_kernel_b": ll_kernel, "ll_form_b": ll_form,
           "a_nni_ll_wall_ms": med(wall_a), "a_nni_ll_device_ms": med(dev_a),
           "b_rebuild_loop_wall_ms": med(wall_b), "b_per_swap_wall_ms": med(wall_b) / max(1, len(swaps)),
           "b_wall_ms_by_call": {key: med([p[key] for p in parts_b]) for key in parts_b[0]},
           "b_without_pattern_upload_wall_ms": med([w - p["set_patterns"] for w, p in zip(wall_b, parts_b)]),
           "a_below_b_without_pattern_upload": bool(med(wall_a) < med([w - p["set_patterns"] for w, p in zip(wall_b, parts_b)])),
           "c_deriv_wall_ms": med(wall_c), "c_deriv_device_ms": med(dev_c),
           "b_over_a_wall": med(wall_b) / med(wall_a), "a_below_b": bool(med(wall_a) < med(wall_b)),
           "a_over_c_device": med(dev_a) / med(dev_c), "a_vs_b_max_rel_diff_of_sums": diff,
           "all_wall_ms": {"a": wall_a, "b": wall_b, "c": wall_c}, "registers": register_counts()}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
