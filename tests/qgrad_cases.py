"""Expected values and cases for the edge pair-sum and rate-matrix-gradient tests (test infrastructure; may use oracle/).

Everything expected here comes from the oracle as it stands: site_edge_expect on arbitrary [C][E][k][k] matrices in
binary128, frechet for the binary128 Frechet matrices, site_ll for the root vector; sums over sites and edges and the
chain rule run in numpy long double."""
import copy
import ctypes

import numpy as np

from phyly_amd import engine as _E, synth

LD = np.longdouble


# ---------------------------------------------------------------- binary128 images of doubles (the oracle's F format)
def q128(a):
    """float64 array -> the oracle's binary128 buffer (two float64-sized words per entry, little endian)"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    bits = a.view(np.uint64).ravel()
    sign = bits >> np.uint64(63)
    ex = (bits >> np.uint64(52)) & np.uint64(0x7FF)
    man = bits & np.uint64((1 << 52) - 1)
    assert np.all((ex != 0) | (man == 0)) and np.all(ex != 0x7FF), "normal numbers and zeros only"
    hi = (sign << np.uint64(63)) | ((ex + np.uint64(16383 - 1023)) << np.uint64(48)) | (man >> np.uint64(4))
    lo = (man & np.uint64(0xF)) << np.uint64(60)
    zero = ex == 0
    hi[zero] = sign[zero] << np.uint64(63)
    out = np.empty(2 * bits.size, dtype=np.uint64)
    out[0::2], out[1::2] = lo, hi
    return out.view(np.float64)


# ---------------------------------------------------------------- cases: model_and_data documents
NINE_TAXON_EDGES = [[0, 1], [0, 2], [0, 3], [1, 4], [1, 5], [2, 6], [2, 7], [6, 8], [6, 9], [3, 10], [3, 11], [10, 12], [10, 13], [11, 14], [14, 15], [14, 16]]


def nine_taxon_doc(S, C, seed, k=4, dense=False, divisor="equilibrium_exit_rate", root="equilibrium_distribution", rate_matrix=None):
    """a 9-taxon tree (leaves 4 5 7 8 9 12 13 15 16) with a three-child root (0), a one-child node (11 -> 14), data on the
    internal node 6 and one ambiguity code; k states, C gamma categories (C = 1: no mixture; C = 5: 4 + invariable)"""
    from helpers import nonreversible_rates
    rng = np.random.default_rng(seed)
    Q = nonreversible_rates(k, rng) if rate_matrix is None else np.asarray(rate_matrix, dtype=float)
    N, E = 17, 16
    leaves = [4, 5, 7, 8, 9, 12, 13, 15, 16]
    defs = np.vstack([np.eye(k), np.ones((1, k)), rng.choice([0.25, 0.5, 1.0], size=(1, k))])
    codes = np.full((S, N), k, dtype=int)                      # missing everywhere ...
    codes[:, leaves] = rng.integers(0, k, (S, len(leaves)))   # ... observed leaves
    codes[:, 6] = np.where(rng.random(S) < 0.5, rng.integers(0, k, S), k)      # data on an internal node
    amb = rng.random((S, len(leaves))) < 0.08
    sub = codes[:, leaves]
    sub[amb] = k + 1
    codes[:, leaves] = sub
    codes[:, 4] = np.where(rng.random(S) < 0.1, k, codes[:, 4])
    md = {"edges": NINE_TAXON_EDGES, "edge_rate_coefficients": [float(v) for v in rng.uniform(0.02, 0.6, E)],
          "rate_matrix": Q.tolist(), "rate_divisor": divisor, "root_prior": root}
    if root is None:
        del md["root_prior"]
    if C > 1:
        md["gamma_rate_mixture"] = dict(gamma_shape=0.7, gamma_categories=4 if C == 5 else C)
        if C == 5:
            md["gamma_rate_mixture"]["invariable_prior"] = 0.15
    if dense:
        md["probability_array"] = defs[codes].tolist()
    else:
        md["character_definitions"] = defs.tolist()
        md["character_data"] = codes.tolist()
    return md


def small_tree_doc(S, k, seed, T=3):
    """a T-taxon caterpillar, k states, one category: the oracle's binary128 work grows with k^3 per Frechet matrix"""
    from helpers import nonreversible_rates
    rng = np.random.default_rng(seed)
    edges, nxt, top = [], 1, 0
    leaves = []
    for t in range(T - 1):
        a, b = nxt, nxt + 1
        nxt += 2
        edges += [[top, a], [top, b]]
        leaves.append(a)
        top = b
    leaves.append(top)
    N = nxt
    defs = np.vstack([np.eye(k), np.ones((1, k))])
    codes = np.full((S, N), k, dtype=int)
    codes[:, leaves] = rng.integers(0, k, (S, len(leaves)))
    return {"edges": edges, "edge_rate_coefficients": [float(v) for v in rng.uniform(0.05, 0.5, len(edges))],
            "rate_matrix": nonreversible_rates(k, rng).tolist(), "rate_divisor": "equilibrium_exit_rate",
            "root_prior": "equilibrium_distribution", "character_definitions": defs.tolist(), "character_data": codes.tolist()}


def mixture_of(md):
    return md.get("gamma_rate_mixture")


def setup_engine(eng, oracle, md, dense=None):
    """tree, model (the product's own K0) and patterns of a document on an Engine -> (m, w) of the oracle"""
    m = oracle.parse_model(md)
    w = oracle.prepare(m)
    k0 = synth.k0_prepare(m.rate_matrix, mixture_of(md), bool(m.use_eq_divisor), m.divisor, m.root_mode == 4 or bool(m.use_eq_divisor))
    rw = k0["pi"] if m.root_mode == 4 else (np.asarray(m.root_custom, dtype=float) if m.root_mode == 2 else None)
    eng.set_tree(m.indptr, m.indices, m.preorder)
    eng.set_model(k0["Qn"], m.edge_rates_csr, k0["cat_rates"], k0["cat_prior"], m.root_mode, rw, Qn_lo=k0["Qn_lo"])
    if dense if dense is not None else "probability_array" in md:
        eng.set_patterns_dense(np.ascontiguousarray(np.transpose(m.B, (1, 2, 0))))
    else:
        eng.set_patterns_codes(np.ascontiguousarray(np.asarray(md["character_data"], dtype=np.uint8).T), np.asarray(md["character_definitions"], dtype=float))
    return m, w


# ---------------------------------------------------------------- oracle W, R, G, root
def _wsum(vals, weights):
    return np.tensordot(np.asarray(weights, dtype=LD), np.asarray(vals, dtype=LD), axes=(0, 0))


def oracle_W(oracle, m, w, weights, nthreads=0, cats=None):
    """W[c][e][i][j] by the issue's definition: the weighted site sum of site_edge_expect with F zero except a 1 at
    (c, i, j) on every edge, coef_mode 0 -> [C][E][k][k] long double (categories not in `cats` stay 0).
    weights None: the per-site terms [S][C][E][k][k], for callers that sum them under several weight vectors."""
    C, E, k = int(w["C"]), m.E, m.k
    W = np.zeros((m.S, C, E, k, k), dtype=LD)
    for c in (range(C) if cats is None else cats):
        for i in range(k):
            for j in range(k):
                F = np.zeros((C, E, k, k))
                F[c, :, i, j] = 1.0
                W[:, c, :, i, j] = oracle.site_edge_expect(m, w, m.B, q128(F), 0, nthreads=nthreads)
    return W if weights is None else _wsum(W, weights)


def oracle_W_factored(oracle, m, w, weights, nthreads=0, precise=2, sites=None):
    """The same W from 2k + 1 oracle calls per category instead of k^2, for state counts where k^2 binary128 up passes
    are out of reach of a test: per site and edge, with F nonzero in category c only,
        x(e_i 1^T) = a_i = p fe[i] (1 . L) / f,   x(1 e_j^T) = b_j = p (fe . 1) L[j] / f,   x(1 1^T) = t = p (fe . 1)(1 . L) / f
    so p fe[i] L[j] / f = a_i b_j / t exactly; the three factors are correctly rounded doubles of binary128 values and
    every term is non-negative, which puts the relative error of each W entry below 4 ulp.  Checked against oracle_W.
    weights None: the per-site terms, as in oracle_W.  precise = 1: the oracle's long-double pass on double P (for state
    counts whose binary128 pass is too slow for a test; the caller holds it against precise = 2 on a few sites);
    sites: a slice of the sites of m."""
    C, E, k = int(w["C"]), m.E, m.k
    B = m.B if sites is None else np.ascontiguousarray(m.B[sites])
    W = np.zeros((B.shape[0], C, E, k, k), dtype=LD)
    for c in range(C):
        def run(F1):
            F = np.zeros((C, E, k, k))
            F[c] = F1
            return np.asarray(oracle.site_edge_expect(m, w, B, q128(F) if precise == 2 else F, 0, nthreads=nthreads, precise=precise), dtype=LD)
        t = run(np.ones((k, k)))
        a = np.stack([run(np.outer(np.eye(k)[i], np.ones(k))) for i in range(k)], axis=2)      # [S][E][k]
        b = np.stack([run(np.outer(np.ones(k), np.eye(k)[j])) for j in range(k)], axis=2)
        with np.errstate(divide="ignore", invalid="ignore"):
            term = np.where(t[:, :, None, None] > 0, a[:, :, :, None] * b[:, :, None, :] / t[:, :, None, None], 0)
        W[:, c] = term
    return W if weights is None else _wsum(W, weights)


def oracle_root(oracle, m, w, weights, per_category=False):
    """root[i] = d/droot_w[i] = sum_s w_s L_i(s) / lhood_s with L_i the site likelihood under the one-hot custom root
    prior e_i -> [k], or per category [C][k] (the workspace cut down to one category, times its prior).
    weights None: the per-site terms [S][C][k] (per_category) or [S][k]."""
    k, C = m.k, int(w["C"])
    ll, _ = oracle.site_ll(m, w, B=m.B, precise=2)
    ll = np.asarray(ll, dtype=LD)
    m1 = copy.copy(m)
    m1.root_mode = 2
    Pq = np.asarray(w["Pq"]).reshape(C, -1)
    out = np.zeros((m.S, C, k), dtype=LD)
    for c in range(C) if per_category else [None]:
        wc = w if c is None else dict(w, C=1, P=np.ascontiguousarray(w["P"][c:c + 1]), Pq=np.ascontiguousarray(Pq[c]), cat_prior=np.ones(1))
        for i in range(k):
            li, _ = oracle.site_ll(m1, dict(wc, root_w=np.eye(k)[i].copy()), B=m.B, precise=2)
            with np.errstate(over="ignore"):
                r = np.exp(np.asarray(li, dtype=LD) - ll)
            out[:, 0 if c is None else c, i] = r * (1 if c is None else LD(w["cat_prior"][c]))
    if weights is not None:
        out = _wsum(out, weights)
    return out if per_category else out[..., 0, :]


def oracle_G(oracle, m, w, weights, nthreads=0):
    """G[i][j] = d/dQn[i][j] from k^2 unit directions: frechet(e_i e_j^T, mul_by_Q=False) + site_edge_expect with
    coef_mode 1 (prior * rate * edge rate), summed over sites and edges"""
    k = m.k
    G = np.zeros((k, k), dtype=LD)
    for i in range(k):
        for j in range(k):
            L = np.zeros((k, k))
            L[i, j] = 1.0
            Fq = oracle.frechet(m, w, L, mul_by_Q=False)
            x = oracle.site_edge_expect(m, w, m.B, Fq, 1, nthreads=nthreads)
            G[i, j] = np.sum(_wsum(x, weights))
    return G


def oracle_G_adjoint(oracle, m, w, W):
    """G = sum_{c,e} s F_{c,e}(W[c][e]^T)^T from the oracle's W and the oracle's binary128 Frechet matrices (rounded to
    double on the way out, 1 ulp): C * E frechet calls instead of k^2 up passes, for large k.  The adjoint identity it
    uses is checked against oracle_G on a small case."""
    C, E, k = int(w["C"]), m.E, m.k
    G = np.zeros((k, k), dtype=LD)
    er = np.asarray(m.edge_rates_csr, dtype=LD)
    cr = np.asarray(w["cat_rates"], dtype=LD)
    for c in range(C):
        for e in range(E):
            req = np.zeros(E, dtype=np.int32)
            req[e] = 1
            Wt = W[c, e].T
            sc = np.max(np.sum(np.abs(Wt), axis=1))
            if sc == 0:
                continue
            F = oracle.frechet(m, dict(w, C=1, cat_rates=np.ascontiguousarray(w["cat_rates"][c:c + 1])), Wt / sc, edge_requested=req, precise=1)
            F = np.asarray(F, dtype=LD).reshape(1, E, k, k)[0, e]
            G += cr[c] * er[e] * sc * F.T
    return G


# ---------------------------------------------------------------- chain rule in long double
def normalised(Q, divisor, want_pi=True):
    """(Qn, pi, d) of a raw rate matrix in long double; divisor: a number or "equilibrium_exit_rate" """
    Q = np.array(Q, dtype=LD)
    k = Q.shape[0]
    np.fill_diagonal(Q, 0)
    np.fill_diagonal(Q, -np.sum(Q, axis=1))
    pi = None
    if want_pi or divisor == "equilibrium_exit_rate":
        A = np.vstack([Q.T[:-1], np.ones((1, k), dtype=LD)])
        b = np.zeros(k, dtype=LD)
        b[-1] = 1
        pi = ld_solve(A, b)
    d = LD(divisor) if divisor != "equilibrium_exit_rate" else -np.sum(pi * np.diag(Q))
    return Q / d, pi, d


def ld_solve(A, b):
    """Gaussian elimination with partial pivoting in long double (numpy.linalg has no long double)"""
    A = np.array(A, dtype=LD)
    b = np.array(b, dtype=LD).reshape(len(A), -1)
    n = len(A)
    for c in range(n):
        p = c + int(np.argmax(np.abs(A[c:, c])))
        A[[c, p]], b[[c, p]] = A[[p, c]], b[[p, c]]
        b[c] /= A[c, c]
        A[c] /= A[c, c]
        for r in range(n):
            if r != c and A[r, c] != 0:
                b[r] -= A[r, c] * b[c]
                A[r] -= A[r, c] * A[c]
    return b if b.shape[1] > 1 else b[:, 0]


def chain(Q, divisor, eq_root, G, root):
    """d/dq_ij (i != j) of f = f(Qn(Q), pi(Q)) from G = df/dQn and root = df/dpi (used only with an equilibrium root
    prior), the formulas of include/plk.h:plk_rate_matrix_chain in long double"""
    Q = np.array(Q, dtype=LD)
    k = Q.shape[0]
    G = np.asarray(G, dtype=LD)
    eq_div = divisor == "equilibrium_exit_rate"
    Qn, pi, d = normalised(Q, divisor, want_pi=eq_root or eq_div)
    grad = (G - np.diag(G)[:, None]) / d
    if eq_root or eq_div:
        Qd = Qn * d
        Z = ld_solve(np.outer(np.ones(k, dtype=LD), pi) - Qd, np.eye(k, dtype=LD))
        v = np.zeros(k, dtype=LD)
        dfdd = LD(0)
        if eq_root:
            v += np.asarray(root, dtype=LD)
        if eq_div:
            dfdd = -np.sum(G * Qn) / d
            v += dfdd * -np.diag(Qd)
        u = Z @ v
        grad = grad + pi[:, None] * (u[None, :] - u[:, None]) + (dfdd * pi[:, None] if eq_div else 0)
    grad = np.array(grad, dtype=LD)
    np.fill_diagonal(grad, 0)
    return grad


def product_chain(Q, divisor, root_mode, G, root):
    """plk_rate_matrix_chain through ctypes -> (rc, grad [k][k], message)"""
    lib = _E.load_library()
    Q = np.ascontiguousarray(Q, dtype=np.float64)
    k = Q.shape[0]

    def dd(x):
        x = np.asarray(x, dtype=LD)
        hi = x.astype(np.float64)
        return np.ascontiguousarray(np.stack([hi, (x - hi.astype(LD)).astype(np.float64)], axis=-1))
    Gd = dd(G)
    rd = dd(root) if root is not None else None
    grad = np.zeros((k, k))
    err = ctypes.create_string_buffer(200)
    eq = divisor == "equilibrium_exit_rate"
    vp = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None
    rc = lib.plk_rate_matrix_chain(k, vp(Q), 1 if eq else 0, 1.0 if eq else float(divisor), int(root_mode), vp(Gd), vp(rd), vp(grad), err, 200)
    return rc, grad, err.value.decode()


def expected_table(oracle, md, site_reduction, nthreads=0, adjoint=False):
    """the table arbplf-rate-matrix-deriv must print: (rows [[i, j, value], ...], G, root) from the oracle alone"""
    m = oracle.parse_model(md)
    w = oracle.prepare(m)
    r_site = oracle.parse_reduction(site_reduction, m.S, "site")
    weights, div = oracle._axis_weights(r_site)          # one weight per site (repeated selections add up), and the divisor
    G = oracle_G(oracle, m, w, weights, nthreads) if not adjoint else oracle_G_adjoint(oracle, m, w, oracle_W_factored(oracle, m, w, weights, nthreads))
    root = oracle_root(oracle, m, w, weights) if m.root_mode == 4 else None
    grad = chain(m.rate_matrix, "equilibrium_exit_rate" if m.use_eq_divisor else m.divisor, m.root_mode == 4, G, root) / LD(div)
    k = m.k
    return [[i, j, grad[i, j]] for i in range(k) for j in range(k) if i != j], G, root
