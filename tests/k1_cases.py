"""Shared cases of tests/test_k1_reference_cpu.py and tests/test_gpu_k1_extremes.py: K1 (P = exp(Qn r_c t_e), dP, d2P, the
Frechet blocks) at extreme branch lengths.  See DESIGN.md section 2, "K1 at the extremes".

The tree is a star: 12 leaves (nodes 0..11) under a root (node 12) that carries data, so that a site showing state i at
the root, state j at leaf e and the missing code elsewhere has, with one rate category, the likelihood
root_w[i] P[e][i][j]: one entry of one matrix.  User edge e = CSR edge e = the edge to leaf e.

The edge rates are the ladder below; its last rung R is chosen per model so that the largest r_c t_e |Qn|_inf is just
under 2^40, the documented limit of K1 (phyly_amd/csrc/plk_k1_check.h)."""
import numpy as np

from helpers import CustomWorkload, nonreversible_rates, tree_workload
from phyly_amd import synth

LADDER = (0.0, 1e-40, 1e-20, 1e-12, 1e-6, 1e-3, 0.1, 1.0, 30.0, 1e3, 1e6, None)       # None: R
MIX = dict(rates=[0.0, 1e-3, 1.0, 50.0], prior=[0.1, 0.2, 0.3, 0.4])
STAR = [[12, leaf] for leaf in range(12)]
ROOT_NODE = 12
LIMIT = 2.0 ** 40
SMALLEST = 1e-250            # no non-zero reference entry below it: no subnormal in any comparison (low words included)

# k -> (zero_frac, root prior, seed).  The k = 4 seed gives a rate matrix with five off-diagonal zeros, one of them an
# entry three steps from the diagonal (1e-130 on the shortest rung); k = 13, 27 and 61 have two-step entries (1e-91)
MODELS = {4: (0.3, "custom", 6156), 13: (0.3, "equilibrium", 6113), 14: (0.3, "none", 6114), 27: (0.3, "uniform", 6127),
          32: (0.3, "none", 6132), 61: (0.5, "none", 6161)}
# The birth chain and the ladder.  With x = lambda / divisor x r_c x t_e the Poisson entries are e^-x x^m / m!.  The rung
# 1e6 under the category rate 50 is inside the limit only if lambda / divisor <= 2^40 / (2 x 50 x 1e6) = 1.1e4, and the
# seven-step entry P_07 on the rung 1e-40 is above SMALLEST only if lambda / divisor >= 4e4 (3e7 under the category rate
# 1e-3): at k = 8 no chain has both.  lambda / divisor = 4096 keeps the whole ladder (R = 2.7e6) and every entry above
# SMALLEST but P_07 on the rung 1e-40 under the categories 1e-3 and 1 (3.8e-280 and 3.8e-259; 2.6e-247 under 50).  Those
# two are compared like every other entry: a double-double keeps its 106 bits while its high word is above
# 2^-1074 x 2^106 = 4e-292, so BIRTH_SMALLEST = 1e-285 is the floor that matters for this model.  On this ladder x is at
# most 410 (entries above 1e-180) or at least 4096: the latter entries are below 1e-1700 (UNDERFLOWN, far beneath the
# subnormals), their doubles are exactly 0 and the device must return exactly 0 as well.
# tests/test_k1_reference_cpu.py checks all of this.
BIRTH_K, BIRTH_LAMBDA, BIRTH_DIVISOR = 8, 1.0, 2.0 ** -12
BIRTH_SMALLEST = 1e-285
UNDERFLOWN = "1e-400"        # compared in mpmath


def qnorm(Qn):
    return float(np.max(np.sum(np.abs(np.asarray(Qn, dtype=float)), axis=1)))


class BirthWorkload(CustomWorkload):
    """the pure-birth chain q_{i,i+1} = lambda with an absorbing last state: reducible, so no equilibrium anywhere; a
    numeric rate divisor and no root prior"""

    def prepare(self):
        if self.k0 is None:
            self.k0 = synth.k0_prepare(self.Q, getattr(self, "rate_mixture", None), False, BIRTH_DIVISOR, False)
        return self.k0

    def json_model(self, codes_host):
        md = CustomWorkload.json_model(self, codes_host)
        md["rate_divisor"] = BIRTH_DIVISOR
        return md


def _shell(k, rates, mixture, nchar, edges=STAR):
    if k == "birth":
        wl = tree_workload(BIRTH_K, edges, rates, root="none", seed=6108, rate_mixture=mixture, nchar=nchar, name="k1 birth chain")
        wl.__class__ = BirthWorkload
        Q = np.zeros((BIRTH_K, BIRTH_K))
        Q[np.arange(BIRTH_K - 1), np.arange(1, BIRTH_K)] = BIRTH_LAMBDA
        wl.Q = Q.tolist()
        return wl
    zero_frac, root, seed = MODELS[k]
    wl = tree_workload(k, edges, rates, root=root, seed=seed, rate_mixture=mixture, nchar=nchar, name="k1 k=%d" % k)
    wl.Q = nonreversible_rates(k, np.random.default_rng(seed + 1), zero_frac).tolist()
    return wl


def top_rung(k, mixture):
    """R: the largest r_c R |Qn|_inf is 2^40 (1 - 2^-20)"""
    probe = _shell(k, [0.1] * 12, mixture, None)
    k0 = probe.prepare()
    return LIMIT * (1.0 - 2.0 ** -20) / (float(np.max(k0["cat_rates"])) * qnorm(k0["Qn"]))


def ladder(k, mixture):
    return [top_rung(k, mixture) if r is None else r for r in LADDER]


def star_workload(k, mixed, nchar=None, rates=None):
    """k: a key of MODELS or "birth"; mixed: the four-category mixture MIX, else one category; nchar: character
    definitions (default k + 1); rates: the 12 edge rates (default: the ladder)"""
    mixture = MIX if mixed else None
    return _shell(k, ladder(k, mixture) if rates is None else rates, mixture, nchar)


def entry_sites(k, triples):
    """codes[N][S] of the sites (i, j, e): state i at the root, state j at leaf e, the missing code elsewhere"""
    triples = np.asarray(triples, dtype=int).reshape(-1, 3)
    codes = np.full((13, len(triples)), k, dtype=np.uint8)
    codes[ROOT_NODE] = triples[:, 0]
    codes[triples[:, 2], np.arange(len(triples))] = triples[:, 1]
    return codes


def all_entries(P):
    """every (i, j, e) whose reference entry P[e][i][j] is not zero (k <= 13)"""
    e, i, j = np.nonzero(P)
    return np.stack([i, j, e], axis=1)


def some_entries(P, seed, smallest=8, random=56):
    """per edge the `smallest` smallest non-zero entries and `random` seeded random non-zero ones (k = 27, 61)"""
    rng = np.random.default_rng(seed)
    out = []
    for e in range(P.shape[0]):
        i, j = np.nonzero(P[e])
        order = np.argsort(P[e][i, j], kind="stable")
        pick = list(order[:smallest])
        rest = order[smallest:]
        if len(rest):
            pick += list(rng.choice(rest, size=min(random, len(rest)), replace=False))
        out += [(i[p], j[p], e) for p in pick]
    return np.array(out, dtype=int)


def ulp_distance(got, ref):
    """|got - ref| in units of ulp(ref), entry by entry; where ref is exactly 0: 0 when got is exactly 0 too, else inf"""
    got, ref = np.asarray(got, dtype=float), np.asarray(ref, dtype=float)
    zero = ref == 0
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.abs(got - ref) / np.spacing(np.abs(np.where(zero, 1.0, ref)))
    return np.where(zero, np.where(got == 0, 0.0, np.inf), d)


# Cherries with unequal ladder edges: six cherries (parents 12..17) under a balanced top (18, 19 -> 12..14, 15..17; root 20)
CHERRY_EDGES = ([[20, 18], [20, 19]] + [[18, 12], [18, 13], [18, 14], [19, 15], [19, 16], [19, 17]] +
                [[12 + n, 2 * n + s] for n in range(6) for s in range(2)])


def cherry_workload(k, mixed):
    """leaf 2n takes rung n, leaf 2n + 1 rung 11 - n; internal edges have rate 0.1"""
    mixture = MIX if mixed else None
    lad = ladder(k, mixture)
    rates = [0.1] * 8 + [lad[n if s == 0 else 11 - n] for n in range(6) for s in range(2)]
    return _shell(k, rates, mixture, None, edges=CHERRY_EDGES)


def cherry_sites(wl, seed):
    """65 sites: 33 seeded random ones and 32 where the two leaves of a cherry differ (the other leaves random)"""
    rng = np.random.default_rng(seed)
    k = wl.k
    codes = np.full((wl.N, 65), k, dtype=np.uint8)
    codes[:12] = rng.integers(0, k, (12, 65))
    for s in range(33, 65):
        n = (s - 33) % 6
        a = int(rng.integers(0, k))
        codes[2 * n, s] = a
        codes[2 * n + 1, s] = (a + 1 + int(rng.integers(0, k - 1))) % k
    return codes


# ------------------------------------------------------------------ values K1 accepts and refuses (plk_k1_check.h)
def _base(k=3, C=2, E=3):
    """a valid model whose |Qn|_inf is exactly 1 (rows -0.5, 0.5 / (k - 1) ...; k = 1: the zero matrix)"""
    Qn = np.zeros((k, k))
    if k > 1:
        Qn[:] = 0.5 / (k - 1)
        np.fill_diagonal(Qn, -0.5)
    return dict(Qn=Qn, Qn_lo=np.zeros((k, k)), er=np.full(E, 0.25), cr=np.linspace(0.5, 1.5, C), cp=np.full(C, 1.0 / C),
                root_mode=2, rw=np.full(k, 1.0 / k))


def _with(base=None, **kw):
    d = dict(base if base is not None else _base())
    for name, (index, value) in kw.items():
        a = np.array(d[name], dtype=float)
        a[index] = value
        d[name] = a
    return d


def check_cases():
    """-> [(name, refused, values, (edge, category) the diagnostic must name or None)]; values: dict(Qn, Qn_lo or None,
    er, cr, cp, root_mode, rw or None)"""
    inf, nan = float("inf"), float("nan")
    out = [("valid", False, _base(), None),
           ("no-low-word-no-root", False, dict(_base(), Qn_lo=None, rw=None, root_mode=1), None),
           ("k1", False, _base(k=1, C=1, E=1), None),
           ("k64-C64", False, _base(k=64, C=64, E=1), None),
           ("negative-zero-rates", False, _with(er=(1, -0.0), cr=(0, -0.0), cp=(0, -0.0)), None),
           ("zero-edge-rate", False, _with(er=(0, 0.0)), None),
           ("root-none-ignores-root-w", False, dict(_with(rw=(0, nan)), root_mode=1), None),
           ("root-uniform-ignores-root-w", False, dict(_with(rw=(0, inf)), root_mode=3), None)]
    for what, v in (("inf", inf), ("minus-inf", -inf), ("nan", nan)):
        out += [("Qn-" + what, True, _with(Qn=((1, 2), v)), None),
                ("Qn-lo-" + what, True, _with(Qn_lo=((2, 0), v)), None),
                ("edge-rate-" + what, True, _with(er=(2, v)), None),
                ("cat-rate-" + what, True, _with(cr=(1, v)), None),
                ("cat-prior-" + what, True, _with(cp=(1, v)), None),
                ("root-w-" + what, True, _with(rw=(2, v)), None),
                ("root-w-equilibrium-" + what, True, dict(_with(rw=(0, v)), root_mode=4), None)]
    out += [("edge-rate-negative", True, _with(er=(0, -1e-300)), None),
            ("cat-rate-negative", True, _with(cr=(0, -1.0)), None),
            ("cat-prior-negative", True, _with(cp=(1, -0.25)), None),
            ("k64-last-entry-nan", True, _with(_base(k=64, C=64, E=1), Qn=((63, 63), nan)), None),
            ("C64-last-rate-inf", True, _with(_base(k=64, C=64, E=1), cr=(63, inf)), None)]
    # the limit: |Qn|_inf = 1, category rates (1, 2^-3): the product is the edge rate itself under category 0
    lim = dict(_base(), cr=np.array([1.0, 0.125]))
    out += [("limit-last-accepted", False, _with(lim, er=(1, LIMIT)), None),
            ("limit-first-refused", True, _with(lim, er=(1, float(np.nextafter(LIMIT, np.inf)))), (1, 0)),
            ("limit-second-category", True, dict(_with(lim, er=(2, LIMIT)), cr=np.array([0.125, 1.0 + 2.0 ** -52])), (2, 1)),
            ("limit-E1", True, dict(_base(E=1), er=np.array([LIMIT * 4])), (0, 0)),
            ("overflowing-product", True, dict(_with(er=(0, 1e308)), cr=np.array([1.0, 2.0])), (0, 0)),        # 1e308 x 2
            ("product-1e200-1e200", True, dict(_base(), er=np.array([0.0, 0.0, 1e200]), cr=np.array([0.0, 1e200])), (2, 1)),
            ("huge-Qn", True, dict(_base(), Qn=_base()["Qn"] * 1e300), (0, 0)),                               # a tiny rate divisor
            ("huge-Qn-zero-rates", False, dict(_base(), Qn=_base()["Qn"] * 1e300, er=np.zeros(3)), None)]
    return out


def check_case_line(name, v):
    """one line of the stand-alone program's input (tests/k1_args_main.c)"""
    k, C, E = len(v["Qn"]), len(v["cr"]), len(v["er"])
    nums = list(np.ravel(v["Qn"]))
    if v["Qn_lo"] is not None:
        nums += list(np.ravel(v["Qn_lo"]))
    nums += list(v["er"]) + list(v["cr"]) + list(v["cp"])
    if v["rw"] is not None:
        nums += list(v["rw"])
    return "%s %d %d %d %d %d %d %s" % (name, k, C, E, v["root_mode"], v["Qn_lo"] is not None, v["rw"] is not None,
                                        " ".join(float(x).hex() for x in nums))
