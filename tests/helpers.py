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

    def prepare(self):
        """K0 through the product host layer; an explicit rate_mixture (rates and prior as given) goes in as the custom
        mixture of host_k0.h"""
        if self.k0 is None and getattr(self, "rate_mixture", None) is not None:
            self.k0 = synth.k0_prepare(self.Q, self.rate_mixture, True, 1.0, True)
        return synth.Workload.prepare(self)

    def setup_engine(self, eng):
        k0 = self.prepare()
        mode, rw = self.root_engine()
        eng.set_tree(self.indptr, self.indices, self.preorder)
        eng.set_model(k0["Qn"], self.edge_rates_csr, k0["cat_rates"], k0["cat_prior"], mode, rw, Qn_lo=k0["Qn_lo"])

    def json_model(self, codes_host):
        md = synth.Workload.json_model(self, codes_host)
        if getattr(self, "rate_mixture", None) is not None:
            md["rate_mixture"] = dict(rates=list(self.rate_mixture["rates"]), prior=list(self.rate_mixture["prior"]))
        if self.root == "none":
            del md["root_prior"]
        elif self.root == "uniform":
            md["root_prior"] = "uniform_distribution"
        elif self.root == "custom":
            md["root_prior"] = self.root_custom.tolist()
        return md

    def _observe(self, codes, salt):
        extra = self.nchar - self.k - 1
        data_nodes = getattr(self, "data_nodes", None)
        if not extra and not self.internal_data and not data_nodes:
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
        if data_nodes:
            codes[list(data_nodes)] = rng.integers(0, self.nchar, (len(data_nodes), codes.shape[1]))
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


def tree_workload(k, edges, edge_rates, *, root, seed, rate_mixture=None, gamma=None, nchar=None, data_nodes=(), name=None):
    """custom_workload on an explicit tree: `edges` [[parent, child], ...] of any shape (unary nodes, multifurcations),
    one rate per edge (0 allowed), either an explicit `rate_mixture` dict(rates, prior) (unequal priors, rate-0
    categories), a `gamma` dict as in synth.Workload.mixture, or neither (one category); `nchar` character definitions
    (identity, the missing row, then rows with fractional entries); `data_nodes` are the internal nodes that carry a
    code at every site.  Q is nonreversible_rates(k)."""
    if root not in ROOTS:
        raise ValueError(root)
    if rate_mixture is not None and gamma is not None:
        raise ValueError("one mixture form at most")
    nchar = k + 1 if nchar is None else nchar
    rng = np.random.default_rng(seed)
    wl = CustomWorkload(T=2, k=k, tree="balanced", model="aa20", seed=seed)       # a shell; tree and model replaced below
    wl.name = name or "tree k=%d E=%d root=%s" % (k, len(edges), root)
    wl.edges = [list(map(int, e)) for e in edges]
    wl.E, wl.N = len(edges), len(edges) + 1
    wl.edge_rates = [float(r) for r in edge_rates]
    if len(wl.edge_rates) != wl.E:
        raise ValueError("one rate per edge")
    wl.indptr, wl.indices, wl.preorder, wl.order = synth.csr_from_edges(wl.edges)
    wl.T = int(np.sum(wl.indptr[1:] == wl.indptr[:-1]))
    wl.edge_rates_csr = np.zeros(wl.E)
    wl.edge_rates_csr[wl.order] = wl.edge_rates
    wl.Q = nonreversible_rates(k, rng).tolist()
    wl.mixture = dict(gamma) if gamma is not None else None
    wl.rate_mixture = rate_mixture
    amb = rng.choice([0.0, 0.25, 0.5, 1.0], size=(nchar - k - 1, k))
    amb[np.arange(nchar - k - 1), rng.integers(0, k, nchar - k - 1)] = 0.75            # never an all-zero row
    wl.defs = np.vstack([np.eye(k), np.ones((1, k)), amb])
    wl.nchar = nchar
    wl.root = root
    wl.root_custom = rng.uniform(0.05, 1.0, k) if root == "custom" else None
    wl.internal_data = False
    wl.data_nodes = tuple(data_nodes)
    if any(wl.indptr[a + 1] == wl.indptr[a] for a in wl.data_nodes):
        raise ValueError("data_nodes are internal nodes")
    wl.k0 = None
    wl._cum = None
    return wl


# The irregular tree of K4_MODELS "irregular" and "wide": 13 leaves (0..12), root 13 with three children (14, 15, leaf 12);
# 14 has three children (16, leaves 4 and 5); 15 is unary (child 19); two cherry parents, 23 (leaves 0, 1; no data; edge
# rates 0.04 and 0.3) and 18 (leaves 2, 3; data of its own); 17 carries data too; the edge 20 -> 21 has rate 0.
IRREGULAR_EDGES = [[13, 14], [13, 15], [13, 12], [14, 16], [14, 4], [14, 5], [16, 6], [16, 17], [17, 7], [17, 18], [18, 2], [18, 3],
                   [15, 19], [19, 8], [19, 20], [20, 9], [20, 21], [21, 10], [21, 22], [22, 11], [22, 23], [23, 0], [23, 1]]
IRREGULAR_RATES = [0.11, 0.07, 0.23, 0.05, 0.31, 0.02, 0.17, 0.09, 0.13, 0.06, 0.21, 0.08,
                   0.12, 0.27, 0.03, 0.19, 0.0, 0.14, 0.1, 0.16, 0.22, 0.04, 0.3]
IRREGULAR_CHERRY = (0, 1)            # leaves of the data-free cherry whose edge rates differ 7.5 x
IRREGULAR_DATA_NODES = (18, 17)

# k = 4 models for tests/test_gpu_k4_variants.py (and the CPU check in tests/test_kernel_family_models.py): what
# the engine-level k = 4 tests on synth.Workload gtr_g4 / hky85 cannot see.  See DESIGN.md section 2.
K4_MODELS = ("irregular", "balanced32", "balanced64", "wide")


def k4_workload(name):
    """irregular:  the irregular tree, rate_mixture rates [0, 0.4, 1.1, 2.7] with prior [0.15, 0.4, 0.05, 0.4], custom
                   root prior, 7 character definitions (identity, missing, two fractional rows)
    balanced32: make_tree(32, "balanced") (stack need 4, the pair-table limit), one rate category, no root prior
    balanced64: make_tree(64, "balanced") (stack need 5: no pair tables), gamma 4 + invariable (C = 5), uniform root prior
    wide:       the irregular tree with 17 definitions (8-bit staged codes, no pair tables or pair messages), two
                categories with prior [0.3, 0.7], equilibrium root prior"""
    if name == "irregular":
        return tree_workload(4, IRREGULAR_EDGES, IRREGULAR_RATES, root="custom", seed=4401, nchar=7, data_nodes=IRREGULAR_DATA_NODES,
                             rate_mixture=dict(rates=[0.0, 0.4, 1.1, 2.7], prior=[0.15, 0.4, 0.05, 0.4]), name="k4 irregular")
    if name == "wide":
        return tree_workload(4, IRREGULAR_EDGES, IRREGULAR_RATES, root="equilibrium", seed=4404, nchar=17, data_nodes=IRREGULAR_DATA_NODES,
                             rate_mixture=dict(rates=[0.5, 1.6], prior=[0.3, 0.7]), name="k4 wide")
    if name in ("balanced32", "balanced64"):
        T = int(name[8:])
        shell = synth.Workload(T=T, k=4, tree="balanced", model="hky85", seed=4400 + T)
        gamma = dict(gamma_shape=0.8, gamma_categories=4, invariable_prior=0.1) if T == 64 else None     # priors 4 x 0.225, 0.1
        return tree_workload(4, shell.edges, shell.edge_rates, root="none" if T == 32 else "uniform", seed=4400 + T, gamma=gamma,
                             name="k4 " + name)
    raise ValueError(name)


# Models for tests/test_gpu_query_variants.py beyond K4_MODELS (which other tests enumerate and which stays as it is)
QUERY_MODEL = "balanced64g3"


def query_workload(name):
    """the models of tests/test_gpu_query_variants.py: K4_MODELS and
    balanced64g3: the balanced64 tree (stack need 5) with a 3-category gamma mixture and the uniform root prior: at most 4
                  categories, so the k = 4 pair-sum and mixture-gradient kernels take it, after k_down_fused4<8>"""
    if name == QUERY_MODEL:
        shell = synth.Workload(T=64, k=4, tree="balanced", model="hky85", seed=4464)
        return tree_workload(4, shell.edges, shell.edge_rates, root="uniform", seed=4467, gamma=dict(gamma_shape=0.6, gamma_categories=3),
                             name="k4 " + name)
    return k4_workload(name)


def numeric_divisor_doc(wl, codes_host):
    """wl.json_model with the rate divisor replaced by a fixed number near the mean exit rate of Q (three decimals): the
    one-category models of mixsens_cases.expectations need a divisor that does not depend on the mixture"""
    md = wl.json_model(codes_host)
    Q = np.array(wl.Q, dtype=float)
    np.fill_diagonal(Q, 0.0)
    md["rate_divisor"] = round(float(np.sum(Q)) / wl.k, 3)
    return md


def deep_workload(rate_mixture=None):
    """the smallest input that reaches the 16-slot k = 4 instantiations: the full binary tree over
    512 unary nodes with one leaf each (N = 1535, stack need 9) and ONE character definition, the all-ones row.  Nodes
    0..510 are the binary tree in heap order, 511..1022 the unary nodes, 1023..1534 the leaves."""
    edges = [[(i - 1) // 2, i] for i in range(1, 1023)] + [[511 + i, 1023 + i] for i in range(512)]
    rng = np.random.default_rng(4416)
    rates = rng.uniform(0.01, 0.3, len(edges))
    rates[rng.choice(len(edges), 20, replace=False)] = 0.0
    wl = tree_workload(4, edges, rates, root="custom", seed=4416, rate_mixture=rate_mixture, name="k4 deep")
    wl.defs, wl.nchar = np.ones((1, 4)), 1
    return wl


def cherry_with_unequal_edges(wl, min_ratio=2.0):
    """(leaf b, leaf c) of the data-free cherry of wl whose two edge rates differ most, by at least min_ratio"""
    best = None
    for a in range(wl.N):
        e0, e1 = wl.indptr[a], wl.indptr[a + 1]
        if e1 - e0 != 2 or a in getattr(wl, "data_nodes", ()):
            continue
        b, c = int(wl.indices[e0]), int(wl.indices[e0 + 1])
        if wl.indptr[b + 1] != wl.indptr[b] or wl.indptr[c + 1] != wl.indptr[c]:
            continue
        r0, r1 = wl.edge_rates_csr[e0], wl.edge_rates_csr[e0 + 1]
        ratio = max(r0, r1) / min(r0, r1)
        if best is None or ratio > best[0]:
            best = (ratio, b, c)
    assert best is not None and best[0] >= min_ratio, best
    return best[1], best[2]


# One model per state count for tests/test_gpu_kernel_families.py (and the CPU check that these models can tell a wrong
# kernel from a right one, tests/test_kernel_family_models.py): every k names the padded width or row-tile count it
# exercises.  C * E * k^3 stays small at large k: the oracle's binary128 exponentials dominate the cost.
FAMILY_MODELS = {
    2: dict(T=10, C=3, invariable=0.2, root="none", ambiguity_rows=1, seed=4112),                   # generic <2>; the seed: a
                                                                                                  # pi with max / min = 2.6 (4102: 1.25)
    3: dict(T=10, C=3, invariable=0.15, root="custom", ambiguity_rows=2, internal_data=True),       # generic <4>
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
    return custom_workload(k, spec.pop("T"), C=spec.pop("C"), root=spec.pop("root"), seed=spec.pop("seed", 4100 + k), **spec)
