#!/usr/bin/env python3
"""HIP-event times of the rate-mixture gradient against the two passes it can be compared with, in one process:
  python tools/time_mixture_deriv.py --config 3 --sites 2000000 [--out profiles/mixture_deriv_cfg3.json]
  (a) plk_mixture_sens: one down pass and one up pass that keeps its 2 C numbers in registers;
  (b) one plk_deriv, sums only (writes and re-reads an [E][n] plane);
  (c) plk_edge_pair_sums, root included: the route to the same numbers before this query, by contracting W.
Every figure is PLK_INFO_LAST_QUERY_NS: HIP events on the engine's stream from the first to the last device operation of
the call; the MEDIAN of --reps repetitions after --warmup untimed calls, with the smallest and largest next to it.  Prints
one JSON line; the kernels' register counts come from the build's saved assembly when it is there."""
import argparse
import datetime
import glob
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from phyly_amd import synth, engine as E   # noqa: E402


def timed(fn, warmup, reps, device_ns):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        fn()
        t.append(device_ns() * 1e-6)
    return dict(median_ms=float(np.median(t)), min_ms=float(np.min(t)), max_ms=float(np.max(t)))


def register_counts():
    out = {}
    for path in glob.glob(os.path.join(ROOT, "phyly_amd", "csrc", "build", "plk_engine-hip-amdgcn-*.s")):
        text = open(path).read()
        for blk in text.split("  - .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            if "mixsens" in name or "k_mix_dir" in name:
                g = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
                out[name] = dict(agpr=int(blk.split("\n")[0]), vgpr=g("vgpr_count"), sgpr=g("sgpr_count"),
                                 scratch_bytes=g("private_segment_fixed_size"), vgpr_spills=g("vgpr_spill_count"))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=3)
    ap.add_argument("--sites", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    wl = synth.Workload(a.config)
    S = a.sites
    eng = E.Engine(0)
    wl.setup_engine(eng)
    eng.set_patterns_codes(wl.simulate(S), wl.defs)
    ns = lambda: eng.info(E.INFO_QUERY_NS)
    res = {}

    def sens():
        res["po"], res["ro"] = eng.mixture_sens()

    def deriv():
        res["d"] = eng.deriv(per_site=False)[1]

    t_a = timed(sens, a.warmup, a.reps, ns)
    kernel = eng.info(E.INFO_MIXTURE_SENS_KERNEL)
    t_b = timed(deriv, a.warmup, a.reps, ns)
    t_c = timed(lambda: eng.edge_pair_sums(), a.warmup, a.reps, ns)
    # the Euler identity on the timed inputs: sum_c r_c rate_out[c] = sum_e t_e (edge sums)
    k0 = wl.prepare()
    lhs = float(np.sum(np.asarray(k0["cat_rates"]) * res["ro"].sum(axis=1)))
    rhs = float(np.sum(np.asarray(wl.edge_rates_csr) * np.asarray(res["d"]).sum(axis=1)))
    out = {"date": datetime.date.today().isoformat(), "box": "one MI355X (gfx950)", "config": a.config, "name": wl.name, "sites": S,
           "states": wl.k, "categories": eng.C, "edges": eng.E, "mixture_sens_kernel": kernel,
           "updown_kernel_b": eng.info(E.INFO_UPDOWN_KERNEL), "pair_sums_kernel_c": eng.info(E.INFO_PAIR_SUMS_KERNEL),
           "timing": "PLK_INFO_LAST_QUERY_NS (HIP events from the first to the last device operation of the call), median of %d "
                     "repetitions after %d untimed calls, same process; sums only" % (a.reps, a.warmup),
           "a_mixture_sens": t_a, "b_deriv": t_b, "c_edge_pair_sums": t_c,
           "a_over_b": t_a["median_ms"] / t_b["median_ms"], "a_over_c": t_a["median_ms"] / t_c["median_ms"],
           "a_not_above_b": bool(t_a["median_ms"] <= t_b["median_ms"]), "a_below_c": bool(t_a["median_ms"] < t_c["median_ms"]),
           "euler_identity_rel_diff": abs(lhs - rhs) / max(abs(lhs), abs(rhs), 1e-300), "registers": register_counts()}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
