"""Shared by test_second_order_host.py (no GPU) and test_gpu_second_order.py: the extended-precision solve the
commands are compared with, and the seeded random documents of the command test.  The second half of the file serves
test_second_order_family_models.py (no GPU) and test_gpu_second_order_families.py: conserved data, the scaled norm, the
long-double reference and the wrong kernels that reference is told from.

random_model() of test_gpu_differential.py is written to stress parsing and the likelihood: 1 to 8 sites, edge rates
and rate-matrix entries that are exactly zero, observations at any node, unary internal nodes without data.  The
reference's own Hessian of such a document is singular or not finite in three cases of four (two consecutive edges
through an unobserved unary node are one parameter; 8 sites do not determine 12 rates).  regular_document() keeps what
the generator drew for the tree, the state count, the rate matrix, the divisor, the root prior and the rate mixture and
redraws the rest so that the rates are identifiable: SITES sites, edge rates in [0.05, 0.5], every off-diagonal rate
at least 0.05, observations at the leaves (a fifth of them missing) and at unary internal nodes only, and a plain
site aggregation.  A stationary root prior under which a reversible model loses one root edge stays as drawn (the
drawn matrices are not reversible)."""
import json

import numpy as np

SITES = 300
SEED = 77
CASES = 20


def reference_solve(H, g):
    """inverse and -H^-1 g in long double, refined until the long double residual stalls"""
    Hl = np.asarray(H, dtype=np.longdouble)
    E = Hl.shape[0]
    X = np.linalg.inv(np.asarray(H, dtype=np.float64)).astype(np.longdouble)
    for _ in range(3):                       # Newton-Schulz in long double: X <- X + X (I - H X)
        X = X + X @ (np.eye(E, dtype=np.longdouble) - Hl @ X)
    return X, -(X @ np.asarray(g, dtype=np.longdouble))


def cond_inf(H, X):
    return float(np.max(np.sum(np.abs(H), axis=1)) * np.max(np.sum(np.abs(X), axis=1)))


def regular_document(rng, x):
    md = x["model_and_data"]
    edges = md["edges"]
    n_nodes, k = len(edges) + 1, len(md["rate_matrix"])
    outdeg = [0] * n_nodes
    for a, _ in edges:
        outdeg[a] += 1
    md["edge_rate_coefficients"] = [round(rng.uniform(0.05, 0.5), 4) for _ in edges]
    for i in range(k):
        for j in range(k):
            if i != j:
                md["rate_matrix"][i][j] = max(md["rate_matrix"][i][j], 0.05)
    if "character_data" in md:
        md["character_data"] = [[rng.randrange(k) if (outdeg[n] == 0 and rng.random() < 0.8) or outdeg[n] == 1 else k
                                 for n in range(n_nodes)] for _ in range(SITES)]
    else:
        pa = []
        for _ in range(SITES):
            site = []
            for n in range(n_nodes):
                r = rng.random()
                if outdeg[n] > 1 or (outdeg[n] == 0 and r < 0.2):
                    site.append([1] * k)
                elif r < 0.7:
                    row = [0] * k
                    row[rng.randrange(k)] = 1
                    site.append(row)
                else:
                    site.append([round(rng.random(), 3) + 0.01 for _ in range(k)])
            pa.append(site)
        md["probability_array"] = pa
    x["site_reduction"] = {"aggregation": rng.choice(["sum", "avg"])}
    return x


def random_documents():
    import random
    from test_gpu_differential import random_model
    rng = random.Random(SEED)
    return [regular_document(rng, random_model(rng, "ll")) for _ in range(CASES)]


def expected(oracle, x):
    """(kappa, E, {command: values} or None) from the oracle's Hessian and gradient of the document"""
    s = json.dumps(x)
    ht, dt = json.loads(oracle.arbplf_hess(s)), json.loads(oracle.arbplf_deriv(s))
    E = len(dt["data"])
    H = np.array([r[-1] for r in ht["data"]]).reshape(E, E)
    g = np.array([r[-1] for r in dt["data"]])
    if not (np.all(np.isfinite(H)) and np.all(np.isfinite(g))) or not np.any(H):
        return np.inf, E, None
    with np.errstate(all="ignore"):
        try:
            X, delta = reference_solve(H, g)
        except np.linalg.LinAlgError:
            return np.inf, E, None
    kappa = cond_inf(H, X)
    if not np.isfinite(kappa):
        return np.inf, E, None
    r = np.array(x["model_and_data"]["edge_rate_coefficients"], dtype=np.longdouble)
    return kappa, E, {"inv_hess": X.reshape(-1), "newton_delta": delta, "newton_update": r + delta}


def counts(kappa, E, want):
    """the kappa-scaled bar shows something: kappa * E * 1e-11 <= 1e-6"""
    return want is not None and kappa * E * 1e-11 <= 1e-6


COMMANDS = ("inv_hess", "newton_delta", "newton_update")


def check_commands(oracle, x):
    """the three commands of the product on document x against expected(); -> True when the case counted"""
    import arbplf
    kappa, E, want = expected(oracle, x)
    s = json.dumps(x)
    counted = counts(kappa, E, want)
    for name in COMMANDS:
        try:
            got = json.loads(getattr(arbplf, "arbplf_" + name)(s))
        except RuntimeError:
            assert not counted, "%s refused a well-conditioned input (kappa %.3g, E %d)" % (name, kappa, E)
            continue
        vals = np.array([r[-1] for r in got["data"]])
        assert np.all(np.isfinite(vals))
        assert got["columns"] == (["first_edge", "second_edge", "value"] if name == "inv_hess" else ["edge", "value"])
        assert len(vals) == (E * E if name == "inv_hess" else E)
        if counted:
            ref = (want["newton_delta"] if name == "newton_update" else want[name]).astype(float)
            scale = np.max(np.abs(ref))             # the update is rates + delta: its error is the delta's
            err = np.max(np.abs(vals - want[name].astype(float)))
            assert err <= 2 * kappa * E * 1e-11 * scale + 1e-300, (name, err, kappa, E, scale)
    return counted


# ---------------------------------------------------------------- second order beyond k = 4
# Shared by test_second_order_family_models.py (no GPU) and test_gpu_second_order_families.py.

FAMILY_KS = (2, 5, 9, 13, 20, 27, 33, 48, 61)       # helpers.FAMILY_MODELS met by the Hessian: K = 2, 8, 16, 16, 32, 32, 64, 64, 64
FAMILY_SIZES = (1, 65, 129)                          # one site, one site past GEN_BLOCK, one past two blocks
MOVES = 1e-6                                         # nni_cases.MOVES: what a wrong variant must move the scaled norm by
EXACT_SITES = 5                                      # sites of every reference that are held to binary128


def conserved_codes(wl, S, seed, keep=0.75):
    """wl.random_codes (ambiguity rows and internal data as the workload draws them) with three quarters of the observed
    states of a site replaced by one state per site.  With unrelated states at the leaves the fastest rate category
    carries the whole site likelihood, and a wrong prior or a permuted category only shifts ll by a constant that the
    derivatives do not see; conserved sites give the slow categories a share."""
    k = wl.k
    codes = wl.random_codes(S, seed=seed, missing_frac=0.1)
    rng = np.random.default_rng([seed, 77])
    base = rng.integers(0, k, S)
    hit = (codes < k) & (rng.random(codes.shape) < keep)
    return np.ascontiguousarray(np.where(hit, base[None, :], codes).astype(np.uint8))


def edge_scale(H_sites, g_sites, w):
    """d[E], d_i = sqrt(sum_s |w_s| (|H_s,ii| + g_s,i^2)) from per-site Hessians [S][E][E] and derivatives [S][E]: the
    curvature edge i sees by itself.  d_i d_j is the natural size of entry (i, j), as entries scale like 1 / (t_i t_j)."""
    H = np.asarray(H_sites, dtype=np.longdouble)
    g = np.asarray(g_sites, dtype=np.longdouble)
    aw = np.abs(np.asarray(w, dtype=np.longdouble))
    diag = np.abs(np.diagonal(H, axis1=1, axis2=2))
    return np.sqrt(np.sum(aw[:, None] * (diag + g * g), axis=0)).astype(float)


def scaled_err(got, want, d):
    """max_ij |got_ij - want_ij| / (d_i d_j); NaN if any entry of got is.  Unlike max|dH| / max|H| it does not change
    when the rate coefficient of an edge is rescaled, so a short edge does not hide every other row."""
    with np.errstate(invalid="ignore"):
        r = np.abs(np.asarray(got, dtype=float) - np.asarray(want, dtype=float)) / np.outer(d, d)
    return float("nan") if np.any(np.isnan(r)) else float(np.max(r))


def weights_with_zeros(S, seed):
    """positive non-integer weights, 15 % of them (rounded) exactly zero"""
    rng = np.random.default_rng([seed, 15])
    wts = rng.uniform(0.3, 2.7, S)
    wts[rng.choice(S, int(round(0.15 * S)), replace=False)] = 0.0
    return wts


class Reference:
    """per-site long-double (precise = 1) Hessians, derivatives and log likelihoods of the oracle for all sites of B[S][N][k],
    the first min(exact, S) Hessians first held to the binary128 ones (precise = 2) at 1e-14 of the largest entry (the
    precedent: balanced64 in test_gpu_k4_variants.py).  ld_gap / ld_gap_scaled keep what that comparison measured."""

    def __init__(self, oracle, m, w, B, exact=EXACT_SITES):
        B = np.ascontiguousarray(B, dtype=np.float64)
        self.H = oracle.site_hess(m, w, B, precise=1)
        self.g = oracle.site_deriv(m, w, B, precise=1)
        self.ll, _ = oracle.site_ll(m, w, B=B, precise=1)
        self.finite = bool(np.all(np.isfinite(self.ll)) and np.all(np.isfinite(self.H)) and np.all(np.isfinite(self.g)))
        n = min(exact, B.shape[0])
        Hq = oracle.site_hess(m, w, B[:n], precise=2)
        self.ld_gap = float(np.max(np.abs(self.H[:n] - Hq)) / np.max(np.abs(Hq)))
        d = edge_scale(Hq, self.g[:n], np.ones(n))
        self.ld_gap_scaled = scaled_err(self.H[:n].sum(axis=0), Hq.sum(axis=0), d) if np.all(d > 0) else float("nan")
        assert self.finite, "a site ll, derivative or Hessian of the oracle is not finite"
        assert self.ld_gap <= 1e-14, self.ld_gap

    def sums(self, wts=None):
        """-> (gradient [E], Hessian [E][E], edge scales d [E], gradient bound) under weights wts (None: ones); the bound is
        the one of test_gpu_k4_variants.test_second_order without its factor: sum_s |w_s| max_i |g_s,i|"""
        S = self.H.shape[0]
        wts = np.ones(S) if wts is None else np.asarray(wts, dtype=float)
        wl = wts.astype(np.longdouble)
        H = (self.H.astype(np.longdouble) * wl[:, None, None]).sum(axis=0).astype(float)
        g = (self.g.astype(np.longdouble) * wl[:, None]).sum(axis=0).astype(float)
        gscale = float(np.sum(np.abs(wts) * np.max(np.abs(self.g), axis=1)))
        return g, H, edge_scale(self.H, self.g, wts), gscale


def weighted_hess(oracle, m, w, B, wts):
    """the long-double Hessian sum of one (possibly wrong) model, NaN entries kept"""
    H = oracle.site_hess(m, w, np.ascontiguousarray(B, dtype=np.float64), precise=1).astype(np.longdouble)
    with np.errstate(invalid="ignore"):
        return (H * np.asarray(wts, dtype=np.longdouble)[:, None, None]).sum(axis=0).astype(float)


MUTANTS = ("categories swapped on one edge", "categories rolled", "Qn transposed", "P transposed", "root weights reversed",
           "internal data dropped")


def mutants(wl, m, w, codes):
    """{name: (w', codes') or a one-line reason why the mutant does not apply to this model}: wrong kernels as references
    of their own, all read by the oracle at precise = 1 (w["P"], w["Qn"]).
    - categories 0 and C - 1 exchanged in P on the edge of largest rate (a stride mistake on one edge),
    - P rolled along the category axis, the category rates with it, so that every category meets its neighbour's prior
      (a category offset in the P / dP / d2P streams); a relabelling, hence nothing, where the priors are all equal,
    - Qn transposed (the Q of r Q P and r^2 Q Q P read by columns),
    - P transposed,
    - the root weights reversed, where the root mode reads them (custom and equilibrium),
    - the data of internal nodes replaced by the missing code, where the model draws any."""
    P, C = w["P"], int(w["C"])
    out = {}
    if C > 1:
        e = int(np.argmax(m.edge_rates_csr))
        Ps = P.copy()
        Ps[[0, C - 1], e] = P[[C - 1, 0], e]
        out[MUTANTS[0]] = (dict(w, P=Ps), codes)
    else:
        out[MUTANTS[0]] = "one category"
    prior = np.asarray(w["cat_prior"])
    if C > 1 and np.max(np.abs(prior - np.roll(prior, 1))) > 0.01:
        out[MUTANTS[1]] = (dict(w, P=np.ascontiguousarray(np.roll(P, 1, axis=0)), cat_rates=np.roll(w["cat_rates"], 1)), codes)
    else:
        out[MUTANTS[1]] = "equal category priors: a roll only relabels the categories"
    out[MUTANTS[2]] = (dict(w, Qn=np.ascontiguousarray(w["Qn"].T)), codes)
    out[MUTANTS[3]] = (dict(w, P=np.ascontiguousarray(P.transpose(0, 1, 3, 2))), codes)
    if m.root_mode in (2, 4):
        out[MUTANTS[4]] = (dict(w, root_w=np.ascontiguousarray(w["root_w"][::-1])), codes)
    else:
        out[MUTANTS[4]] = "root prior %s: no root weights are read" % wl.root
    leaf = wl.indptr[1:] == wl.indptr[:-1]
    if np.any(codes[~leaf] != wl.k):
        dropped = codes.copy()
        dropped[~leaf] = wl.k
        out[MUTANTS[5]] = (w, dropped)
    else:
        out[MUTANTS[5]] = "no data on internal nodes"
    return out
