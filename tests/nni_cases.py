"""Nearest-neighbour interchanges for the tests of plk_nni_ll / arbplf-nni: the Python enumeration of the swaps of a tree,
the rewriting of a model document into the swapped tree, the oracle reference of a swap, and the deliberately wrong
variants ("teeth") that the references must tell from the right one.

A swap is a pair of edges (a, b), a = (v -> c), b = (u -> s), v a child of u, s != v.  The swapped tree has a = (u -> c)
and b = (v -> s): only the parents of the two entries of `edges` change; rates, data and every other entry stay.
User indices are positions in the document's `edges`; CSR indices are positions in the CSR `indices` array
(csr = order[user], as oracle.parse_model and synth.csr_from_edges number them)."""
import numpy as np

import mixsens_cases
from phyly_amd import synth

LD = np.longdouble
SITE_TOL = 1e-12          # |got - want| <= SITE_TOL * max(1, |want|): the project's bar for per-site log likelihoods
SUM_TOL = 1e-12           # |hi + lo - long double sum| <= SUM_TOL * |sum|: the bar tests/test_gpu_ll.py holds plk_ll sums to
MOVES = 1e-6              # what a swap, and every wrong variant of it, must move some site's ll by

# Swaps that move no site's ll (user indices), left out of the GPU comparison of values: on the irregular tree the edge
# 20 -> 21 has rate 0 and neither node carries data, so 20 and 21 share their state and it makes no difference which of
# the two a subtree hangs from: the children 10 and 22 of 21 exchanged with the leaf 9 of 20.  2 of 24 swaps; the tree of
# `wide` is the same.  tests/test_nni_cases_cpu.py asserts that these are all.
STILL_SWAPS = {"irregular": [(17, 15), (18, 15)], "wide": [(17, 15), (18, 15)]}


# ---------------------------------------------------------------- enumeration
def in_edges(edges):
    """node -> (user edge into it, parent)"""
    return {int(c): (e, int(p)) for e, (p, c) in enumerate(edges)}


def why_no_swap(edges, a, b, into=None):
    """None when (a, b) is a swap of the tree of `edges` (user indices), else the reason; into: in_edges(edges) when the
    caller has it"""
    E = len(edges)
    if not (isinstance(a, (int, np.integer)) and isinstance(b, (int, np.integer))):
        return "edge indices must be integers"
    if not (0 <= a < E and 0 <= b < E):
        return "edge index out of range"
    if a == b:
        return "the same edge twice"
    into = in_edges(edges) if into is None else into
    v, u, s = int(edges[a][0]), int(edges[b][0]), int(edges[b][1])
    if v not in into:
        return "the first edge starts at the root"
    if into[v][1] != u:
        return "the first edge does not start at a child of the second edge's upper node"
    if s == v:
        return "the second edge ends where the first starts"
    return None


def swaps_user(edges):
    """every swap of the tree in user indices, ordered by (a, b): the definition, edge b tried among the edges that start
    where a's upper node hangs"""
    into = in_edges(edges)
    out_edges = {}
    for e, (p, _) in enumerate(edges):
        out_edges.setdefault(int(p), []).append(e)
    out = []
    for a in range(len(edges)):
        v = int(edges[a][0])
        if v in into:
            out += [(a, b) for b in out_edges[into[v][1]] if why_no_swap(edges, a, b, into) is None]
    return out


def swaps_csr(indptr, indices):
    """every swap of a CSR tree in CSR edge indices, ordered by (a, b) (what plk_nni_swaps must return)"""
    N = len(indptr) - 1
    parent = {}
    for p in range(N):
        for idx in range(indptr[p], indptr[p + 1]):
            parent[int(indices[idx])] = (idx, p)
    out = []
    for a in range(len(indices)):
        v = next(p for p in range(N) if indptr[p] <= a < indptr[p + 1])
        if v not in parent:
            continue
        u = parent[v][1]
        out += [(a, b) for b in range(indptr[u], indptr[u + 1]) if int(indices[b]) != v]
    return out


def user_to_csr(edges, pairs):
    order = synth.csr_from_edges([list(map(int, e)) for e in edges])[3]
    return np.array([[order[a], order[b]] for a, b in pairs], dtype=np.int32).reshape(-1, 2)


def csr_to_user(edges, pairs):
    order = synth.csr_from_edges([list(map(int, e)) for e in edges])[3]
    inv = {c: u for u, c in enumerate(order)}
    return [(inv[int(a)], inv[int(b)]) for a, b in pairs]


# ---------------------------------------------------------------- rewriting
def swap_edges(edges, a, b):
    why = why_no_swap(edges, a, b)
    if why:
        raise ValueError("edges (%r, %r) are no swap: %s" % (a, b, why))
    new = [list(map(int, e)) for e in edges]
    new[a][0], new[b][0] = int(edges[b][0]), int(edges[a][0])       # a = (u -> c), b = (v -> s)
    return new


def swap_doc(md, a, b):
    """the model document of the swapped tree: the parents of edges[a] and edges[b] rewritten, everything else as it is;
    ValueError for a pair that is no swap"""
    new = swap_edges(md["edges"], a, b)
    out = dict(md)
    out["edges"] = new
    return out


# ---------------------------------------------------------------- oracle references
class Reference:
    """The oracle on one document: the current tree prepared once (binary128 exponentials), every swapped tree parsed
    from its rewritten document.  Each edge keeps its rate, so the transition matrices of a rewritten document are those
    of the original, edge by edge; they are moved to the new CSR positions instead of being exponentiated again
    (tests/test_nni_cases_cpu.py checks that against oracle.prepare of the rewritten document)."""

    def __init__(self, oracle, md):
        self.oracle, self.md = oracle, md
        self.m = oracle.parse_model(md)
        self.w = oracle.prepare(self.m)
        self._ll = None
        self._cache = {}

    def current(self):
        if self._ll is None:
            self._ll = self.oracle.site_ll(self.m, self.w, B=self.m.B, precise=1)[0]
        return self._ll

    def model(self, md2, P_user=None):
        """(m, w) of a rewritten document; P_user [C][E][k][k] by USER edge (default: those of the original)"""
        md2 = dict(md2)                                   # the tree is what changed: one site is enough to parse it; the
        for key in ("character_data", "probability_array"):   # observations B of the original serve every rewritten tree
            if key in md2:
                md2[key] = md2[key][:1]
        m2 = self.oracle.parse_model(md2)
        m2.B = self.m.B
        if P_user is None:
            P_user = self.P_user()
        w2 = dict(self.w)
        P2 = np.empty_like(self.w["P"])
        P2[:, m2.order] = P_user
        w2["P"] = np.ascontiguousarray(P2)
        return m2, w2

    def P_user(self):
        return self.w["P"][:, self.m.order].copy()

    def swap(self, a, b):
        """site log likelihoods of the swapped tree (user indices), long double traversal"""
        key = (int(a), int(b))
        if key not in self._cache:
            m2, w2 = self.model(swap_doc(self.md, a, b))
            self._cache[key] = self.oracle.site_ll(m2, w2, B=m2.B, precise=1)[0]
        return self._cache[key]

    # ---- the teeth: each a plausible mistake of an implementation, as a reference of its own
    def wrong_rates_stay(self, a, b):
        """the rate stays with the position instead of travelling with the subtree: the matrices of a and b exchanged"""
        P = self.P_user()
        P[:, [a, b]] = P[:, [b, a]]
        m2, w2 = self.model(swap_doc(self.md, a, b), P)
        return self.oracle.site_ll(m2, w2, B=m2.B, precise=1)[0]

    def wrong_data_dropped(self, a, b):
        """the data of v dropped"""
        v = int(self.md["edges"][a][0])
        m2, w2 = self.model(swap_doc(self.md, a, b))
        B = m2.B.copy()
        B[:, v, :] = 1.0
        return self.oracle.site_ll(m2, w2, B=B, precise=1)[0]

    def wrong_sibling_left_out(self, a, b):
        """c's other siblings left out of v's product: their subtrees send the all-ones message"""
        edges = self.md["edges"]
        v, c = int(edges[a][0]), int(edges[a][1])
        kids = {}
        for p, ch in edges:
            kids.setdefault(int(p), []).append(int(ch))
        below = []
        stack = [w for w in kids.get(v, []) if w != c]
        while stack:
            x = stack.pop()
            below.append(x)
            stack += kids.get(x, [])
        m2, w2 = self.model(swap_doc(self.md, a, b))
        B = m2.B.copy()
        B[:, below, :] = 1.0
        return self.oracle.site_ll(m2, w2, B=B, precise=1)[0], below

    def wrong_categories_exchanged(self, a, b):
        """two categories exchanged on edge a"""
        P = self.P_user()
        C = P.shape[0]
        if C < 2:
            return None
        P[[0, C - 1], a] = P[[C - 1, 0], a]
        m2, w2 = self.model(swap_doc(self.md, a, b), P)
        return self.oracle.site_ll(m2, w2, B=m2.B, precise=1)[0]


def moved(x, y):
    """largest |x - y| over the sites (inf where exactly one is -inf, 0 where both are)"""
    x, y = np.asarray(x, float), np.asarray(y, float)
    both = np.isneginf(x) & np.isneginf(y)
    with np.errstate(invalid="ignore"):
        d = np.where(both, 0.0, np.abs(x - y))
    return float(np.max(d)) if d.size else 0.0


def site_err(got, want):
    """largest |got - want| / max(1, |want|); -inf must meet -inf"""
    got, want = np.asarray(got, float), np.asarray(want, float)
    inf = np.isneginf(want)
    if not np.array_equal(inf, np.isneginf(got)):
        return np.inf
    if np.all(inf):
        return 0.0
    g, w = got[~inf], want[~inf]
    return float(np.max(np.abs(g - w) / np.maximum(1.0, np.abs(w))))


def weighted_sum(ll, wt=None):
    """long double host sum of w_s ll_s, a weight of exactly 0 dropping its term whatever it is (plk_ll's rule)"""
    ll = np.asarray(ll, dtype=LD)
    if wt is None:
        return np.sum(ll)
    wt = np.asarray(wt, dtype=LD)
    keep = wt != 0
    return np.sum(wt[keep] * ll[keep])


def six_decade_weights(S, seed):
    """signed weights over six decades, one of them exactly 0"""
    rng = np.random.default_rng(seed)
    w = rng.choice([-1.0, 1.0], S) * 10.0 ** rng.uniform(-3, 3, S)
    if S > 2:
        w[S // 3] = 0.0
    return w


# ---------------------------------------------------------------- documents
def workload_doc(wl, S, seed=1):
    """model_and_data of a helpers workload on S random sites (leaves, ambiguity codes and internal data as the workload
    draws them)"""
    return wl.json_model(wl.random_codes(S, seed=seed))


def ladder_doc(T, S, seed, k=4, C=2, leaf_scale=1.0):
    """ladder (caterpillar) tree of T leaves with edge rates near 1 and two rate categories; leaf_scale < 1 scales the
    observation rows: 200 leaves at 1e-4 put every site likelihood far below 2^-1022, which only carried-over scale
    factors survive"""
    md = mixsens_cases.caterpillar_doc(T, S, seed, k=k, C=C, leaf_scale=leaf_scale)
    rng = np.random.default_rng(seed + 1)
    md = dict(md)
    md["edge_rate_coefficients"] = rng.uniform(0.8, 1.2, len(md["edges"])).tolist()
    return md


def sample_swaps(edges, n, seed, spread=False):
    """n swaps (user indices) of the tree, seeded; always with one under the root, one with a leaf c and one with a leaf s
    where the tree has them; spread: evenly along the canonical list instead of at random"""
    allsw = swaps_user(edges)
    if len(allsw) <= n:
        return allsw
    into = in_edges(edges)
    parents = {int(p) for p, _ in edges}
    root = next(p for p in parents if p not in into)
    first = []
    for want in (lambda a, b: int(edges[b][0]) == root, lambda a, b: int(edges[a][1]) not in parents,
                 lambda a, b: int(edges[b][1]) not in parents):
        hit = [sw for sw in allsw if want(*sw) and sw not in first]
        if hit:
            first.append(hit[0])
    rest = [sw for sw in allsw if sw not in first]
    if spread:
        pick = [rest[i] for i in np.linspace(0, len(rest) - 1, n - len(first)).astype(int)]
    else:
        rng = np.random.default_rng(seed)
        pick = [rest[i] for i in sorted(rng.choice(len(rest), n - len(first), replace=False))]
    return first + pick
