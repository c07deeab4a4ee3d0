#!/usr/bin/env python3
"""HIP-event times of the rate-matrix gradient against the two things it can be compared with:
  python tools/time_rate_matrix_deriv.py --config 3 --sites 2000000 [--out profiles/rate_matrix_deriv_cfg3.json]
  (a) plk_rate_matrix_sens: one down pass, one pair-sum up pass, one Frechet K1 run, G and root summed;
  (b) the same G through the interface the engine had before: k^2 unit directions through plk_edge_expect_multi with
      PLK_COEF_PRIOR_RATE_EDGE, four per call where the k = 4 kernels carry four edge forms, sums only (k = 4 only);
  (c) one plk_deriv, sums only.
Every figure is PLK_INFO_LAST_QUERY_NS: HIP events on the engine's stream from the first to the last device operation of
the call, mean of --reps repetitions after one untimed call.  Prints one JSON line; the kernels' register counts come from
the build's saved assembly when it is there."""
import argparse
import datetime
import glob
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from phyly_amd import synth, engine as E   # noqa: E402


def timed(fn, reps, device_ns):
    fn()
    wall = dev = 0.0
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        wall += time.perf_counter() - t0
        dev += device_ns() * 1e-9
    return wall / reps * 1e3, dev / reps * 1e3


def register_counts():
    out = {}
    for path in glob.glob(os.path.join(ROOT, "phyly_amd", "csrc", "build", "plk_engine-hip-amdgcn-*.s")):
        text = open(path).read()
        for blk in text.split("  - .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            if "pairsums" in name:
                g = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
                out[name] = dict(agpr=int(blk.split("\n")[0]), vgpr=g("vgpr_count"), sgpr=g("sgpr_count"),
                                 scratch_bytes=g("private_segment_fixed_size"), vgpr_spills=g("vgpr_spill_count"))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=3)
    ap.add_argument("--sites", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    wl = synth.Workload(a.config)
    S, k = a.sites, wl.k
    eng = E.Engine(0)
    wl.setup_engine(eng)
    eng.set_patterns_codes(wl.simulate(S), wl.defs)
    ns = lambda: eng.info(E.INFO_QUERY_NS)
    res = {}

    def sens():
        res["G"] = eng.rate_matrix_sens()[0]

    wall_a, t_a = timed(sens, a.reps, ns)
    kernel = eng.info(E.INFO_PAIR_SUMS_KERNEL)
    out = {"date": datetime.date.today().isoformat(), "box": "one MI355X (gfx950)", "config": a.config, "name": wl.name, "sites": S,
           "states": k, "categories": eng.C, "edges": eng.E, "pair_sums_kernel": kernel,
           "timing": "PLK_INFO_LAST_QUERY_NS (HIP events from the first to the last device operation of the call), mean of %d "
                     "repetitions after one untimed call; sums only, no per-site output" % a.reps,
           "a_rate_matrix_sens_ms": t_a, "wall_ms": {"a": wall_a}}
    if k == 4:
        Ls = np.zeros((16, 4, 4))
        for i in range(4):
            for j in range(4):
                Ls[4 * i + j, i, j] = 1.0
        acc = [0]

        def directions():
            acc[0] = 0
            Gd = np.zeros((4, 4))
            for b in range(4):
                _, sums = eng.edge_expect_multi(Ls[4 * b:4 * b + 4], E.COEF_PRIOR_RATE_EDGE, per_site=False)
                acc[0] += ns()
                Gd[b] = np.asarray(sums).reshape(4, eng.E, 2).sum(axis=(1, 2))
            res["Gd"] = Gd

        wall_b, t_b = timed(directions, a.reps, lambda: acc[0])
        G = res["G"][..., 0] + res["G"][..., 1]
        out.update(b_unit_directions_ms=t_b, b_over_a=t_b / t_a, a_below_b=bool(t_a < t_b),
                   a_vs_b_max_rel_diff=float(np.max(np.abs(G - res["Gd"])) / np.max(np.abs(G))))
        out["wall_ms"]["b"] = wall_b
    wall_c, t_c = timed(lambda: eng.deriv(per_site=False), a.reps, ns)
    out.update(c_deriv_ms=t_c, a_over_c=t_a / t_c, updown_kernel_c=eng.info(E.INFO_UPDOWN_KERNEL), registers=register_counts())
    out["wall_ms"]["c"] = wall_c
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
