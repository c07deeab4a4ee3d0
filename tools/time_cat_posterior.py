#!/usr/bin/env python3
"""HIP-event times of the rate-category posterior query against the two things it can be compared with:
  python tools/time_cat_posterior.py --config 3 --sites 2000000 [--out profiles/catpost_cfg3.json]
  (a) plk_cat_posterior, device-side sums only (no per-site plane leaves the device), the edge rates set anew before
      every repetition so that its one K1 is inside the timed window, as the C K1 runs of (b) are;
  (b) the same numbers without the query: C one-category plk_set_model + per-site plk_ll calls;
  (c) plk_ll on the C++ interpreter (PLK_OPT_PAIR_TABLES = 0, PLK_OPT_FUSED_ASM = 0, variant 3): the same traversal
      without the extra stores, edge rates set anew before every repetition as in (a).
Prints one JSON line; the kernel's register counts come from the build's saved assembly when it is there."""
import argparse
import ctypes
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
    """-> (mean wall ms, mean HIP-event ms of the engine's device work) of fn() over reps calls, after one untimed call;
    device_ns() reads the engine's event time of what the last fn() queued.  Every call is synchronous."""
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
            if "k_ll_fused4_catpost" in name:
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
    S = a.sites
    k0 = wl.prepare()
    C = k0["C"]
    eng = E.Engine(0)
    wl.setup_engine(eng)
    eng.set_patterns_codes(wl.simulate(S), wl.defs)
    lib = eng._lib
    psum, rsum = (ctypes.c_double * (2 * C))(), (ctypes.c_double * 2)()

    def query():
        eng.update_edge_rates(wl.edge_rates_csr)
        eng._check(lib.plk_cat_posterior(eng._h, None, None, psum, rsum))

    wall_a, t_a = timed(query, a.reps, lambda: eng.info(E.INFO_CAT_POSTERIOR_NS))
    kernel = eng.info(E.INFO_CAT_POSTERIOR_KERNEL)
    site_ll = np.empty(S)
    acc = [0]

    def per_category():
        # the events of plk_ll cover its own device work (formats, K1's tables, traversal); K1 inside plk_set_model and the
        # copy of the per-site values are in the wall time only, so the event figure flatters (b)
        acc[0] = 0
        for c in range(C):
            eng.set_model(k0["Qn"], wl.edge_rates_csr, k0["cat_rates"][c:c + 1], [1.0], E.ROOT_EQUILIBRIUM, k0["pi"], Qn_lo=k0["Qn_lo"])
            eng._check(lib.plk_ll(eng._h, ctypes.c_void_p(site_ll.ctypes.data), E.HOST, None))
            acc[0] += eng.info(E.INFO_LL_TOTAL_NS)

    wall_b, t_b = timed(per_category, a.reps, lambda: acc[0])
    variant_b = eng.info(E.INFO_LL_VARIANT)
    # the mixture model again (the tree and the patterns stay)
    eng.set_model(k0["Qn"], wl.edge_rates_csr, k0["cat_rates"], k0["cat_prior"], E.ROOT_EQUILIBRIUM, k0["pi"], Qn_lo=k0["Qn_lo"])
    eng.set_option(E.OPT_PAIR_TABLES, 0)
    eng.set_option(E.OPT_FUSED_ASM, 0)

    def ll_cpp():
        eng.update_edge_rates(wl.edge_rates_csr)
        eng.ll(per_site=False)

    wall_c, t_c = timed(ll_cpp, a.reps, lambda: eng.info(E.INFO_LL_TOTAL_NS))
    variant_c = eng.info(E.INFO_LL_VARIANT)
    out = {"date": datetime.date.today().isoformat(), "config": a.config, "name": wl.name, "sites": S, "categories": C,
           "cat_posterior_kernel": kernel,
           "timing": "HIP events of the engine around its device work, mean of %d repetitions after one untimed; (a) and (c) "
                     "include one K1 per repetition, (b) C traversals with their table builds but not the K1 inside "
                     "plk_set_model nor the copy of the per-site values, which are in wall_ms only" % a.reps,
           "a_cat_posterior_sums_ms": t_a, "a_sites_per_s": S / (t_a * 1e-3),
           "b_per_category_set_model_ll_ms": t_b, "b_ll_variant": variant_b,
           "c_ll_cpp_interpreter_ms": t_c, "c_ll_variant": variant_c,
           "wall_ms": {"a": wall_a, "b": wall_b, "c": wall_c},
           "b_over_a": t_b / t_a, "a_over_c": t_a / t_c,
           "a_faster_than_b": {"events": t_a < t_b, "wall": wall_a < wall_b},
           "registers": register_counts()}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
