"""Shared by test_second_order_host.py (no GPU) and test_gpu_second_order.py: the extended-precision solve the
commands are compared with, and the seeded random documents of the command test.

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
