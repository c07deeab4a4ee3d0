"""Shared helpers for the parity tests (test infrastructure; may use oracle/)."""
import json
import os

import numpy as np

from phyly_amd import engine as _E, synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def oracle_model(oracle, workload, codes_host):
    """Oracle Model + prepared workspace for a synth.Workload and codes[N][S]."""
    md = workload.json_model(codes_host[:, :1])
    m = oracle.parse_model(md)
    w = oracle.prepare(m)
    return m, w


def oracle_site_ll(oracle, workload, codes_host, precise=1, nthreads=0):
    m, w = oracle_model(oracle, workload, codes_host)
    codes_sn = np.ascontiguousarray(codes_host.T)
    ll, used = oracle.site_ll(m, w, codes=codes_sn, defs=workload.defs, precise=precise, nthreads=nthreads)
    return ll


def rel_err(got, want, floor=1.0):
    got, want = np.asarray(got, float), np.asarray(want, float)
    return np.max(np.abs(got - want) / np.maximum(np.abs(want), floor))


def load_json(path):
    with open(path) as f:
        return json.load(f)


ROOTS = ("equilibrium", "uniform", "none", "custom")


def nonreversible_rates(k, rng, zero_frac=0.1):
    """k x k raw rate matrix: off-diagonal entries exp(N(0, 1)), about zero_frac of them set to zero (as in codon
    models) but never the cycle i -> i + 1 (mod k), so the chain stays irreducible.  Neither symmetric nor reversible:
    pi is not uniform and no P is symmetric."""
    Q = np.exp(rng.standard_normal((k, k)))
    Q[rng.random((k, k)) < zero_frac] = 0.0
    idx = np.arange(k)
    Q[idx, (idx + 1) % k] = np.exp(rng.standard_normal(k))
    np.fill_diagonal(Q, 0.0)
    return Q


class CustomWorkload(synth.Workload):
    """synth.Workload whose engine set-up and JSON model honour a root prior other than the equilibrium one, and whose
    data may hold ambiguity codes at the leaves and codes on internal nodes (built by custom_workload)"""

    def root_engine(self):
        if self.root == "equilibrium":
            return _E.ROOT_EQUILIBRIUM, self.prepare()["pi"]
        if self.root == "custom":
            return _E.ROOT_CUSTOM, self.root_custom
        return (_E.ROOT_UNIFORM if self.root == "uniform" else _E.ROOT_NONE), None

    def setup_engine(self, eng):
        k0 = self.prepare()
        mode, rw = self.root_engine()
        eng.set_tree(self.indptr, self.indices, self.preorder)
        eng.set_model(k0["Qn"], self.edge_rates_csr, k0["cat_rates"], k0["cat_prior"], mode, rw, Qn_lo=k0["Qn_lo"])

    def json_model(self, codes_host):
        md = synth.Workload.json_model(self, codes_host)
        if self.root == "none":
            del md["root_prior"]
        elif self.root == "uniform":
            md["root_prior"] = "uniform_distribution"
        elif self.root == "custom":
            md["root_prior"] = self.root_custom.tolist()
        return md

    def _observe(self, codes, salt):
        extra = self.nchar - self.k - 1
        if not extra and not self.internal_data:
            return codes
        rng = np.random.default_rng([self.seed, salt, codes.shape[1]])
        codes = codes.copy()
        leaf = self.indptr[1:] == self.indptr[:-1]
        if extra:
            hit = (rng.random(codes.shape) < 0.1) & leaf[:, None]
            codes[hit] = (self.k + 1 + rng.integers(0, extra, codes.shape))[hit]
        if self.internal_data:
            inner = np.flatnonzero(~leaf)[::3]
            codes[inner] = rng.integers(0, self.nchar, (len(inner), codes.shape[1]))
        return codes

    def simulate(self, S, site0=0, device=None):
        if device is not None:
            raise ValueError("CustomWorkload simulates on the host only")
        return self._observe(synth.Workload.simulate(self, S, site0), 1)

    def random_codes(self, S, seed=1, missing_frac=0.05):
        return self._observe(synth.Workload.random_codes(self, S, seed, missing_frac), 2 + seed)


def custom_workload(k, T, *, C, root, seed, tree="yule", invariable=0.0, ambiguity_rows=0, internal_data=False):
    """A k-state, T-taxon workload on a non-reversible model (nonreversible_rates) with C rate categories from
    gamma_rate_mixture (one of them the rate-0 category P = I when invariable > 0), root prior `root` (one of ROOTS;
    "custom" draws a positive vector), character definitions identity + the all-ones missing row + `ambiguity_rows`
    rows with fractional entries (nchar > k + 1), and with internal_data, codes on a third of the internal nodes."""
    if root not in ROOTS:
        raise ValueError(root)
    ncat = C - (1 if invariable > 0 else 0)
    if ncat < 1:
        raise ValueError("C must leave at least one gamma category")
    rng = np.random.default_rng(seed)
    wl = CustomWorkload(T=T, k=k, tree=tree, model="aa20", seed=seed)     # tree and branch lengths; Q replaced below
    wl.name = "custom k=%d T=%d C=%d root=%s" % (k, T, C, root)
    wl.Q = nonreversible_rates(k, rng).tolist()
    wl.mixture = None
    if C > 1:
        wl.mixture = dict(gamma_shape=float(rng.choice([0.4, 0.8, 1.7])), gamma_categories=int(ncat))
        if invariable > 0:
            wl.mixture["invariable_prior"] = float(invariable)
    amb = rng.choice([0.0, 0.25, 0.5, 1.0], size=(ambiguity_rows, k))
    amb[np.arange(ambiguity_rows), rng.integers(0, k, ambiguity_rows)] = 0.75      # never an all-zero row
    wl.defs = np.vstack([np.eye(k), np.ones((1, k)), amb])
    wl.nchar = k + 1 + ambiguity_rows
    wl.root = root
    wl.root_custom = rng.uniform(0.05, 1.0, k) if root == "custom" else None
    wl.internal_data = internal_data
    wl.k0 = None
    wl._cum = None
    return wl


# One model per state count for tests/test_gpu_kernel_families.py (and the CPU check that these models can tell a wrong
# kernel from a right one, tests/test_kernel_family_models.py): every k names the padded width or row-tile count it
# exercises.  C * E * k^3 stays small at large k: the oracle's binary128 exponentials dominate the cost.
FAMILY_MODELS = {
    5: dict(T=14, C=4, invariable=0.2, root="custom", ambiguity_rows=2, internal_data=True),      # generic <8>
    8: dict(T=12, C=3, root="none"),
    9: dict(T=12, C=3, invariable=0.15, root="uniform"),                                          # vec K = 16 / MFMA T = 1
    13: dict(T=10, C=4, root="custom", ambiguity_rows=2, internal_data=True),
    16: dict(T=10, C=3, root="none", tree="balanced"),
    17: dict(T=10, C=3, invariable=0.1, root="equilibrium", ambiguity_rows=1),                    # vec K = 20 / MFMA T = 2
    20: dict(T=9, C=4, invariable=0.2, root="custom", internal_data=True),
    21: dict(T=9, C=3, root="uniform"),                                                           # vec K = 32 / MFMA T = 2
    27: dict(T=8, C=3, invariable=0.2, root="none", ambiguity_rows=2, internal_data=True),
    32: dict(T=8, C=3, root="custom"),
    33: dict(T=7, C=3, invariable=0.2, root="equilibrium", ambiguity_rows=2),                      # MFMA T = 3
    48: dict(T=6, C=2, root="none", internal_data=True),
    49: dict(T=6, C=2, invariable=0.25, root="uniform", ambiguity_rows=1),                        # MFMA T = 4
    61: dict(T=6, C=2, root="custom"),
    64: dict(T=6, C=2, invariable=0.2, root="equilibrium", internal_data=True),
}


def family_workload(k):
    spec = dict(FAMILY_MODELS[k])
    return custom_workload(k, spec.pop("T"), C=spec.pop("C"), root=spec.pop("root"), seed=4100 + k, **spec)
