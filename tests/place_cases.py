"""Placements for the tests of plk_place_ll / arbplf-place: the rewriting of a model document into the tree with one query
taxon attached to one edge, the oracle reference of a placement, and the deliberately wrong variants ("teeth") that the
references must tell from the right one.

A placement onto the user edge e = (u -> b) with rate r_e, `split` and `pendant` replaces e by (u -> N) with rate
fl(split r_e) and appends (N -> b) with rate fl(fl(1 - split) r_e) and (N -> N + 1) with rate pendant: node N is new and
has no data, node N + 1 is the query's leaf.  Every other edge, node and datum stays.
User indices are positions in the document's `edges`; CSR indices are csr = order[user] (nni_cases.user_to_csr)."""
import numpy as np

import nni_cases
from nni_cases import LD, MOVES, SITE_TOL, SUM_TOL, moved, site_err, six_decade_weights, weighted_sum   # noqa: F401 (re-exported)
from phyly_amd import synth

TEETH = ("ab_exchanged", "whole_edge_above", "no_pendant", "attached_at_u", "siblings_left_out", "wrong_character")

# Placements on which a tooth cannot bite (user edge indices), asserted to be all of them by
# tests/test_place_cases_cpu.py.  The irregular tree (K4_MODELS irregular and wide): the edge 20 -> 21 (index 16) has rate
# 0, so both of its parts are the identity whatever the split and exchanging them or giving the upper part the whole edge
# changes nothing; under such an edge the query hangs from u as well as from the new node when neither carries data.  The
# sibling tooth has nothing to drop where u has one child: 15 -> 19 (index 12), and on `balanced32` no edge at all.
STILL = {
    ("irregular", "ab_exchanged"): [16], ("wide", "ab_exchanged"): [16],
    ("irregular", "whole_edge_above"): [16], ("wide", "whole_edge_above"): [16],
    ("irregular", "attached_at_u"): [16], ("wide", "attached_at_u"): [16],
    ("irregular", "siblings_left_out"): [12], ("wide", "siblings_left_out"): [12],
}


def edge_rates(md, e, split, pendant):
    """(upper, lower, pendant) rate coefficients of the three new edges, rounded as the engine rounds them"""
    r = float(md["edge_rate_coefficients"][e])
    return float(split) * r, (1.0 - float(split)) * r, float(pendant)


def missing_code(md):
    """(definitions, index of an all-ones definition), one appended when the document has none"""
    defs = [list(map(float, row)) for row in md["character_definitions"]]
    for c, row in enumerate(defs):
        if all(v == 1.0 for v in row):
            return defs, c
    return defs + [[1.0] * len(defs[0])], len(defs)


def place_doc(md, e, query_obs, split, pendant):
    """the model document of the tree with the query attached to user edge e; query_obs: per site a character index
    (character_data documents) or a row of k probabilities (probability_array documents)"""
    edges = [list(map(int, x)) for x in md["edges"]]
    N = len(edges) + 1
    u, b = edges[e]
    up, low, pen = edge_rates(md, e, split, pendant)
    out = dict(md)
    edges[e] = [u, N]
    out["edges"] = edges + [[N, b], [N, N + 1]]
    rates = [float(v) for v in md["edge_rate_coefficients"]]
    rates[e] = up
    out["edge_rate_coefficients"] = rates + [low, pen]
    if "character_data" in md:
        defs, miss = missing_code(md)
        out["character_definitions"] = defs
        out["character_data"] = [list(row) + [miss, int(q)] for row, q in zip(md["character_data"], query_obs)]
    else:
        k = len(md["rate_matrix"])
        out["probability_array"] = [list(row) + [[1.0] * k, [float(v) for v in q]] for row, q in zip(md["probability_array"], query_obs)]
    return out


def attach_at_u_doc(md, e, query_obs, pendant):
    """a wrong tree: the edge stays whole and the query hangs from its upper node"""
    edges = [list(map(int, x)) for x in md["edges"]]
    N = len(edges) + 1
    out = dict(md)
    out["edges"] = edges + [[edges[e][0], N]]
    out["edge_rate_coefficients"] = [float(v) for v in md["edge_rate_coefficients"]] + [float(pendant)]
    if "character_data" in md:
        out["character_data"] = [list(row) + [int(q)] for row, q in zip(md["character_data"], query_obs)]
    else:
        out["probability_array"] = [list(row) + [[float(v) for v in q]] for row, q in zip(md["probability_array"], query_obs)]
    return out


def obs_rows(md, query_obs):
    """[S][k] observation rows of a query given as place_doc takes it"""
    if "character_data" in md:
        return np.asarray(md["character_definitions"], dtype=float)[np.asarray(query_obs, dtype=int)]
    return np.asarray(query_obs, dtype=float)


def csr_edges(md, user_edges):
    order = synth.csr_from_edges([list(map(int, e)) for e in md["edges"]])[3]
    return np.array([order[e] for e in user_edges], dtype=np.int32)


# ---------------------------------------------------------------- oracle references
class Reference:
    """The oracle on one document: the current tree prepared once (binary128 exponentials).  A placement is parsed from its
    rewritten document; unchanged edges keep the matrices of the original, moved to their new CSR positions, and the
    three new matrices come from the oracle's preparation of a three-edge document with the new rates (cached by rate)."""

    def __init__(self, oracle, md):
        self.oracle, self.md = oracle, md
        self.m = oracle.parse_model(md)
        self.w = oracle.prepare(self.m)
        self.k = self.m.k
        self._ll = None
        self._P = {}

    def current(self):
        if self._ll is None:
            self._ll = self.oracle.site_ll(self.m, self.w, B=self.m.B, precise=1)[0]
        return self._ll

    def P_user(self):
        return self.w["P"][:, self.m.order].copy()

    def matrices(self, rates):
        """[C][k][k] transition matrix of every rate coefficient in `rates`"""
        todo = sorted({float(r) for r in rates} - set(self._P))
        if todo:
            mini = {key: v for key, v in self.md.items() if key not in ("character_data", "character_definitions", "probability_array")}
            mini["edges"] = [[0, i + 1] for i in range(len(todo))]
            mini["edge_rate_coefficients"] = todo
            mini["probability_array"] = [[[1.0] * self.k] * (len(todo) + 1)]
            m3 = self.oracle.parse_model(mini)
            P3 = self.oracle.prepare(m3)["P"]
            for i, r in enumerate(todo):
                self._P[r] = P3[:, m3.order[i]].copy()
        return [self._P[float(r)] for r in rates]

    def _tree(self, md2):
        md2 = dict(md2)
        for key in ("character_data", "probability_array"):       # the tree is what is parsed: one site is enough
            if key in md2:
                md2[key] = md2[key][:1]
        return self.oracle.parse_model(md2)

    def _run(self, m2, P_user2, B2):
        w2 = dict(self.w)
        P2 = np.empty((self.w["C"], m2.E, self.k, self.k))
        P2[:, m2.order] = P_user2
        w2["P"] = np.ascontiguousarray(P2)
        return self.oracle.site_ll(m2, w2, B=np.ascontiguousarray(B2), precise=1)[0]

    def place(self, e, query_obs, split, pendant, tooth=None):
        """site log likelihoods with the query attached to user edge e, long double traversal; tooth: one of TEETH"""
        assert tooth is None or tooth in TEETH
        S, k = self.m.B.shape[0], self.k
        if tooth == "wrong_character":
            query_obs = [(int(q) + 1) % len(self.md["character_definitions"]) for q in query_obs]
        X = obs_rows(self.md, query_obs)
        B = self.m.B
        if tooth == "siblings_left_out":
            u, b = map(int, self.md["edges"][e])
            kids = {}
            for p, c in self.md["edges"]:
                kids.setdefault(int(p), []).append(int(c))
            below, stack = [], [w for w in kids[u] if w != b]
            while stack:
                x = stack.pop()
                below.append(x)
                stack += kids.get(x, [])
            B = B.copy()
            B[:, below, :] = 1.0
        Pu = self.P_user()
        if tooth == "attached_at_u":
            m2 = self._tree(attach_at_u_doc(self.md, e, query_obs, pendant))
            D, = self.matrices([float(pendant)])
            return self._run(m2, np.concatenate([Pu, D[:, None]], axis=1), np.concatenate([B, X[:, None, :]], axis=1))
        m2 = self._tree(place_doc(self.md, e, query_obs, split, pendant))
        up, low, pen = edge_rates(self.md, e, split, pendant)
        A, Bm, D = self.matrices([up, low, pen])
        eye = np.broadcast_to(np.eye(k), A.shape)
        if tooth == "ab_exchanged":
            A, Bm = Bm, A
        elif tooth == "whole_edge_above":
            A, Bm = Pu[:, e], eye
        elif tooth == "no_pendant":
            D = eye
        P2 = np.concatenate([Pu, Bm[:, None], D[:, None]], axis=1)
        P2[:, e] = A
        B2 = np.concatenate([B, np.ones((S, 1, k)), X[:, None, :]], axis=1)
        return self._run(m2, P2, B2)


# ---------------------------------------------------------------- queries and edge samples
def queries(md, wl_codes, seed):
    """three query taxa for a character_data document, [3][S] character indices: random codes, all missing, a copy of one
    leaf's column; wl_codes: the document's character_data as an array [S][N]"""
    rng = np.random.default_rng(seed)
    S = wl_codes.shape[0]
    defs, miss = missing_code(md)
    assert miss < len(md["character_definitions"]), "the document needs an all-ones definition"
    parents = {int(p) for p, _ in md["edges"]}
    leaf = min(int(c) for _, c in md["edges"] if int(c) not in parents)
    return np.stack([rng.integers(0, len(md["character_definitions"]), S), np.full(S, miss), wl_codes[:, leaf]]).astype(np.uint8)


def edge_kinds(md):
    """user edge -> set of the kinds the issue names: root (under the root), leaf, data (into an internal node with data at
    some site), multi (under a node with more than two children), zero (rate 0)"""
    edges = [list(map(int, e)) for e in md["edges"]]
    parents = [p for p, _ in edges]
    children = {c for _, c in edges}
    root = next(p for p in parents if p not in children)
    miss = missing_code(md)[1] if "character_data" in md else None
    data = np.asarray(md["character_data"]) if "character_data" in md else None
    out = {}
    for e, (p, c) in enumerate(edges):
        kinds = set()
        if p == root:
            kinds.add("root")
        if c not in parents:
            kinds.add("leaf")
        elif data is not None and np.any(data[:, c] != miss):
            kinds.add("data")
        if parents.count(p) > 2:
            kinds.add("multi")
        if float(md["edge_rate_coefficients"][e]) == 0.0:
            kinds.add("zero")
        out[e] = kinds
    return out


def sample_edges(md, n, seed, spread=False):
    """n user edges, seeded, always with one of every kind of edge_kinds the tree has; spread: evenly along the list"""
    kinds = edge_kinds(md)
    E = len(md["edges"])
    if E <= n:
        return list(range(E))
    first = []
    for kind in ("root", "leaf", "data", "multi", "zero"):
        hit = [e for e in range(E) if kind in kinds[e] and e not in first]
        if hit and not any(kind in kinds[e] for e in first):
            first.append(hit[0])
    rest = [e for e in range(E) if e not in first]
    if spread:
        pick = [rest[i] for i in np.linspace(0, len(rest) - 1, n - len(first)).astype(int)]
    else:
        rng = np.random.default_rng(seed)
        pick = [rest[i] for i in sorted(rng.choice(len(rest), n - len(first), replace=False))]
    return first + pick


def workload_doc(wl, S, seed=1):
    return nni_cases.workload_doc(wl, S, seed)


def ladder_doc(T, S, seed, k=4, C=2, leaf_scale=1.0):
    return nni_cases.ladder_doc(T, S, seed, k=k, C=C, leaf_scale=leaf_scale)
