"""Subtree prune-and-regraft moves for the tests of plk_spr_ll / arbplf-spr: the Python enumeration of the moves of a tree,
the rewriting of a model document into the moved tree, the oracle reference of a move, and the deliberately wrong
variants ("teeth") that the references must tell from the right one.

A move is a pair of edges (p, e), p = (w -> x) the pruned edge and e = (u -> b) the target, e neither p nor an edge of
the subtree below x.  With N the number of nodes of the document the moved tree has edges[e] = [u, N], edges[p] = [N, x]
and one appended edge [N, b]; the rates are fl(split r_e) for e, fl(fl(1 - split) r_e) for the appended edge and r_p for
p; node N is new and has no data (a missing-code column).  Every other edge, node and datum stays; w keeps its data and
loses one child.
User indices are positions in the document's `edges`; CSR indices are csr = order[user] (nni_cases.user_to_csr)."""
import numpy as np

import nni_cases
import place_cases
from nni_cases import LD, MOVES, SITE_TOL, SUM_TOL, moved, site_err, six_decade_weights, weighted_sum   # noqa: F401 (re-exported)
from place_cases import missing_code
from phyly_amd import synth

TEETH = ("lb_of_current_tree_on_path", "fu_of_current_tree_below_w", "message_of_p_kept_at_w", "ab_exchanged", "attached_at_u",
         "sc_w_dropped")
KINDS = ("x_leaf", "x_internal", "w_root", "sibling", "into_w", "above_w", "below_sibling", "far", "w_multi", "data", "zero")


# ---------------------------------------------------------------- the tree of a document
class Tree:
    def __init__(self, edges):
        self.edges = [(int(p), int(c)) for p, c in edges]
        self.E = len(self.edges)
        self.into = {c: (e, p) for e, (p, c) in enumerate(self.edges)}
        self.kids = {}
        for e, (p, c) in enumerate(self.edges):
            self.kids.setdefault(p, []).append(c)
        self.root = next(p for p, _ in self.edges if p not in self.into)
        self.has_data = None                                   # filled by move_kinds
        self.pos, self.size = {}, {}
        order, stack = [], [self.root]
        while stack:
            y = stack.pop()
            self.pos[y] = len(order)
            order.append(y)
            stack += reversed(self.kids.get(y, []))
        for y in reversed(order):
            self.size[y] = 1 + sum(self.size[c] for c in self.kids.get(y, []))

    def is_below(self, y, x):
        """y is x or below x"""
        return self.pos[x] <= self.pos[y] < self.pos[x] + self.size[x]

    def below(self, x):
        """x and every node below it"""
        out, stack = set(), [x]
        while stack:
            y = stack.pop()
            out.add(y)
            stack += self.kids.get(y, [])
        return out

    def path(self, w):
        """w, its parent, ..., the root"""
        out = [w]
        while out[-1] in self.into:
            out.append(self.into[out[-1]][1])
        return out


def why_no_move(edges, p, e, tree=None):
    """None when (p, e) is a move of the tree of `edges` (user indices), else the reason"""
    E = len(edges)
    if not (isinstance(p, (int, np.integer)) and isinstance(e, (int, np.integer))):
        return "edge indices must be integers"
    if not (0 <= p < E and 0 <= e < E):
        return "edge index out of range"
    if p == e:
        return "the target is the pruned edge"
    t = Tree(edges) if tree is None else tree
    if t.is_below(t.edges[e][0], t.edges[p][1]):
        return "the target lies below the pruned edge"
    return None


def moves_user(edges):
    """every move of the tree in user indices, ordered by (p, e): the definition"""
    t = Tree(edges)
    out = []
    for p in range(t.E):
        x = t.edges[p][1]
        out += [(p, e) for e in range(t.E) if e != p and not t.is_below(t.edges[e][0], x)]
    return out


def moves_csr(indptr, indices):
    """every move of a CSR tree in CSR edge indices, ordered by (p, e) (what plk_spr_moves must return)"""
    N = len(indptr) - 1
    edges = [(a, int(indices[idx])) for a in range(N) for idx in range(indptr[a], indptr[a + 1])]
    return moves_user(edges)


def user_to_csr(edges, pairs):
    return nni_cases.user_to_csr(edges, pairs)


def csr_to_user(edges, pairs):
    return nni_cases.csr_to_user(edges, pairs)


# ---------------------------------------------------------------- rewriting
def part_rates(md, e, split):
    """(upper, lower) rate coefficients of the two parts of the target edge, rounded as the engine rounds them"""
    r = float(md["edge_rate_coefficients"][e])
    return float(split) * r, (1.0 - float(split)) * r


def _with_new_columns(md, out, n_new):
    """n_new data-free nodes appended to the observations of `out`"""
    if "character_data" in md:
        defs, miss = missing_code(md)
        out["character_definitions"] = defs
        out["character_data"] = [list(row) + [miss] * n_new for row in md["character_data"]]
    else:
        k = len(md["rate_matrix"])
        out["probability_array"] = [list(row) + [[1.0] * k] * n_new for row in md["probability_array"]]
    return out


def move_doc(md, p, e, split):
    """the model document of the moved tree; ValueError for a pair that is no move"""
    why = why_no_move(md["edges"], p, e)
    if why:
        raise ValueError("edges (%r, %r) are no move: %s" % (p, e, why))
    edges = [list(map(int, x)) for x in md["edges"]]
    N = len(edges) + 1
    (u, b), x = edges[e], edges[p][1]
    up, low = part_rates(md, e, split)
    out = dict(md)
    edges[e] = [u, N]
    edges[p] = [N, x]
    out["edges"] = edges + [[N, b]]
    rates = [float(v) for v in md["edge_rate_coefficients"]]
    rates[e] = up
    out["edge_rate_coefficients"] = rates + [low]
    return _with_new_columns(md, out, 1)


def attached_at_u_doc(md, p, e):
    """a wrong tree: the target edge stays whole and the pruned subtree hangs from its upper node"""
    edges = [list(map(int, x)) for x in md["edges"]]
    edges[p] = [edges[e][0], edges[p][1]]
    return dict(md, edges=edges)


# ---------------------------------------------------------------- oracle references
class Reference(place_cases.Reference):
    """The oracle on one document: the current tree prepared once (binary128 exponentials).  A move is parsed from its
    rewritten document; unchanged edges keep the matrices of the original, moved to their new CSR positions, and the
    matrices of the two parts of the target edge come from the oracle's preparation of a small document with the new rates
    (cached by rate)."""

    def __init__(self, oracle, md):
        super().__init__(oracle, md)
        self.tree = Tree(md["edges"])
        self._moves = {}

    def move(self, p, e, split, tooth=None):
        """site log likelihoods of the moved tree (user indices), long double traversal; tooth: one of TEETH, None where
        the tooth has nothing to say about this move"""
        assert tooth is None or tooth in TEETH
        key = (int(p), int(e), float(split), tooth)
        if key not in self._moves:
            self._moves[key] = self._move(int(p), int(e), float(split), tooth)
        return self._moves[key]

    def _move(self, p, e, split, tooth):
        t, k = self.tree, self.k
        S = self.m.B.shape[0]
        (w, x), (u, b) = t.edges[p], t.edges[e]
        Pu = self.P_user()
        if tooth == "attached_at_u":
            m2 = self._tree(attached_at_u_doc(self.md, p, e))
            return self._run(m2, Pu, self.m.B)
        up, low = part_rates(self.md, e, split)
        A, Bm = self.matrices([up, low])
        if tooth == "ab_exchanged":
            A, Bm = Bm, A
        md2 = move_doc(self.md, p, e, split)
        P2 = np.concatenate([Pu, Bm[:, None]], axis=1)
        P2[:, e] = A
        B2 = np.concatenate([self.m.B, np.ones((S, 1, k))], axis=1)
        ghost = {"lb_of_current_tree_on_path": t.is_below(w, b), "fu_of_current_tree_below_w": t.is_below(u, w),
                 "message_of_p_kept_at_w": True}
        if tooth in ghost:
            # the vectors of the CURRENT tree in place of those of the pruned one: the pruned subtree is still seen at w.
            # As a tree: a copy of the subtree of x, edge by edge with its rates and data, left hanging at w.
            if not ghost[tooth]:
                return None
            sub = [ed for ed in range(t.E) if t.edges[ed][1] in t.below(x)]      # p and the edges below x
            N2 = len(md2["edges"]) + 1
            copy = {y: N2 + i for i, y in enumerate(sorted(t.below(x)))}
            md2 = dict(md2)
            md2["edges"] = md2["edges"] + [[w if ed == p else copy[t.edges[ed][0]], copy[t.edges[ed][1]]] for ed in sub]
            md2["edge_rate_coefficients"] = md2["edge_rate_coefficients"] + [float(self.md["edge_rate_coefficients"][ed]) for ed in sub]
            for key in ("character_data", "probability_array"):
                if key in md2:
                    md2[key] = [list(row) + [row[y] for y in sorted(t.below(x))] for row in md2[key]]
            P2 = np.concatenate([P2, Pu[:, sub]], axis=1)
            B2 = np.concatenate([B2, self.m.B[:, sorted(t.below(x))]], axis=1)
        if tooth == "sc_w_dropped":
            # were w a rescaled node, its factor would be 2^-ilogb(largest entry of w's vector) per site and category; a
            # pass that books the factor and forms L'_w without it is off by that power of two in every category
            m2 = self._tree(md2)
            C = self.w["C"]
            terms = np.empty((C, S), dtype=LD)
            ex = self.scale_exponents(w)
            for c in range(C):
                wc = dict(self.w, C=1, cat_prior=np.ones(1), P=np.ascontiguousarray(self.w["P"][c:c + 1]))
                one = place_cases.Reference._run(_Shim(self.oracle, wc, k), m2, P2[c:c + 1], B2)
                terms[c] = np.asarray(one, dtype=LD) + np.log(LD(self.w["cat_prior"][c])) + ex[:, c].astype(LD) * np.log(LD(2.0))
            top = np.max(terms, axis=0)
            with np.errstate(invalid="ignore", divide="ignore"):
                out = np.where(np.isneginf(top), top, top + np.log(np.sum(np.exp(terms - np.where(np.isneginf(top), 0, top)), axis=0)))
            return np.asarray(out, dtype=float)
        return self._run(self._tree(md2), P2, B2)

    def scale_exponents(self, w):
        """[S][C] ilogb(max_i L_w[i]) of the current tree, 0 where the vector is 0"""
        mx = self.down_vector(w).max(axis=2)
        with np.errstate(divide="ignore"):
            ex = np.floor(np.log2(mx))
        return np.where(np.isfinite(ex), ex, 0.0)

    def down_vector(self, y):
        """[S][C][k] the down vector of node y in the current tree (plain doubles; it is only used for its exponent)"""
        t, Pu, B = self.tree, self.P_user(), self.m.B
        C = Pu.shape[0]
        out = np.repeat(B[:, None, y, :], C, axis=1).astype(float)
        for c in t.kids.get(y, []):
            L = self.down_vector(c)
            ed = t.into[c][0]
            msg = np.einsum("cij,scj->sci", Pu[:, ed], L)
            const = np.all(L == L[:, :, :1], axis=2, keepdims=True)
            out = out * np.where(const, L, msg)
        return out


class _Shim:
    """what place_cases.Reference._run reads of a reference, for one category on its own"""

    def __init__(self, oracle, w, k):
        self.oracle, self.w, self.k = oracle, w, k


# ---------------------------------------------------------------- samples
def move_kinds(md, p, e, t=None):
    """the kinds of KINDS a move has; t: Tree(md["edges"]) when the caller has it"""
    t = Tree(md["edges"]) if t is None else t
    (w, x), (u, b) = t.edges[p], t.edges[e]
    rates = md["edge_rate_coefficients"]
    kinds = {"x_internal" if x in t.kids else "x_leaf"}
    if w == t.root:
        kinds.add("w_root")
    if u == w:
        kinds.add("sibling")
    elif b == w:
        kinds.add("into_w")
    elif t.is_below(w, b):
        kinds.add("above_w")
    elif t.is_below(u, w):
        kinds.add("below_sibling")
    elif not t.is_below(w, u):
        kinds.add("far")
    if len(t.kids[w]) > 2:
        kinds.add("w_multi")
    if "character_data" in md:
        if t.has_data is None:
            miss = missing_code(md)[1]
            t.has_data = np.any(np.asarray(md["character_data"]) != miss, axis=0)
        if t.has_data[w] or t.has_data[u]:
            kinds.add("data")
    if float(rates[p]) == 0.0 or float(rates[e]) == 0.0:
        kinds.add("zero")
    return kinds


def tree_kinds(md, moves=None):
    """the kinds the listed moves have between them (default: every move of the tree)"""
    t = Tree(md["edges"])
    moves = moves_user(md["edges"]) if moves is None else moves
    return set().union(*(move_kinds(md, p, e, t) for p, e in moves)) if moves else set()


def sample_moves(md, n, seed, spread=False):
    """n moves (user indices), seeded, always with one of every kind of KINDS the tree has; spread: evenly along the list"""
    allmv = moves_user(md["edges"])
    if len(allmv) <= n:
        return allmv
    rng = np.random.default_rng(seed)
    t = Tree(md["edges"])
    kinds = {}
    first, have = [], set()
    for kind in KINDS:
        if kind in have:
            continue
        for i in rng.permutation(len(allmv)):
            mv = allmv[int(i)]
            if mv not in kinds:
                kinds[mv] = move_kinds(md, *mv, t)
            if kind in kinds[mv] and mv not in first:
                first.append(mv)
                have |= kinds[mv]
                break
    rest = [mv for mv in allmv if mv not in first]
    if spread:
        pick = [rest[i] for i in np.linspace(0, len(rest) - 1, n - len(first)).astype(int)]
    else:
        pick = [rest[i] for i in sorted(rng.choice(len(rest), n - len(first), replace=False))]
    return first + pick


def workload_doc(wl, S, seed=1):
    return nni_cases.workload_doc(wl, S, seed)


def ladder_doc(T, S, seed, k=4, C=2, leaf_scale=1.0):
    return nni_cases.ladder_doc(T, S, seed, k=k, C=C, leaf_scale=leaf_scale)
