"""Queries for arbplf-dwell / -trans / -em-update whose likelihood is positive by construction, the documents whose
likelihood is zero, and the small models with known answers (tests/test_gpu_expect.py; the CPU check that these lists
are what they claim, tests/test_expect_cases_cpu.py).

random_query draws a model from test_gpu_differential.random_model (whose stream other tests depend on, so it stays as
it is) and the third-axis reduction of the query.  About a third of those draws have a site of likelihood zero: an
observed state changes across a rate-0 edge, or Q's zero pattern forbids an observed transition.  feasible_query keeps
the draw's tree, rates, mixture, root prior, divisor and reductions and replaces the data: every site gets a latent
state per node, drawn down the tree, and every observation is positive at the latent state.  With the cycle
i -> i + 1 (mod k) forced into Q every state reaches every state, so exp(Q t) > 0 for t > 0 and pi > 0, a child across
a rate-0 edge repeats its parent, and the latent path alone has positive probability under any category of positive
rate.  Zero edge rates, rate-0 categories and the other structural zeros of Q stay."""
import copy
import random

from test_gpu_differential import random_model

KINDS = ("dwell", "trans", "em_update")
SEEDS = {"dwell": 44, "trans": 55, "em_update": 66}
NCASES = 60
BLOCK = 20
NBLOCKS = NCASES // BLOCK
FORMS = ("missing", "exact", "ambiguous")


def random_query(rng, kind):
    """random_model plus the state / pair reduction of the query (the draw the random differential always used)"""
    x = random_model(rng, "deriv")          # model + optional site / edge reductions
    md = x["model_and_data"]
    k = len(md["rate_matrix"])

    def red(n):
        r = rng.random()
        if r < 0.3:
            return None
        out = {}
        if rng.random() < 0.6:
            out["selection"] = [rng.randrange(n) for _ in range(rng.randrange(1, n + 2))]
        m = len(out.get("selection", range(n)))
        r = rng.random()
        if r < 0.3:
            out["aggregation"] = "sum"
        elif r < 0.45:
            out["aggregation"] = "avg"
        elif r < 0.75:
            out["aggregation"] = [round(rng.uniform(-1, 2), 3) for _ in range(m)]
        return out

    if kind == "dwell":
        r = red(k)
        if r is not None:
            x["state_reduction"] = r
    elif kind == "trans":
        r = rng.random()
        if r < 0.25:
            pass
        elif r < 0.4:
            x["trans_reduction"] = {"aggregation": rng.choice(["sum", "avg"])}
        else:
            pairs = [[rng.randrange(k), rng.randrange(k)] for _ in range(rng.randrange(1, 6))]
            tr = {"selection": pairs}
            r = rng.random()
            if r < 0.3:
                tr["aggregation"] = "sum"
            elif r < 0.6:
                tr["aggregation"] = [round(rng.uniform(-1, 2), 3) for _ in pairs]
            x["trans_reduction"] = tr
    else:
        x.pop("edge_reduction", None)
        sr = x.get("site_reduction") or {}
        if "aggregation" not in sr:
            sr["aggregation"] = "sum"
        x["site_reduction"] = sr
    return x


def top_down(edges):
    """(root, [(parent, child, edge index), ...] with every parent before its children)"""
    below = {}
    for e, (p, c) in enumerate(edges):
        below.setdefault(p, []).append((c, e))
    root = ({p for p, _ in edges} - {c for _, c in edges}).pop()
    out, stack = [], [root]
    while stack:
        p = stack.pop()
        for c, e in below.get(p, []):
            out.append((p, c, e))
            stack.append(c)
    return root, out


def _force_cycle(md):
    Q = md["rate_matrix"]
    k = len(Q)
    for i in range(k):
        if Q[i][(i + 1) % k] == 0:
            Q[i][(i + 1) % k] = 0.3


def _more_structural_zeros(rng, md):
    """one more zero off the cycle in a quarter of the draws with k >= 3"""
    Q = md["rate_matrix"]
    k = len(Q)
    if k >= 3 and rng.random() < 0.25:
        i = rng.randrange(k)
        j = rng.choice([j for j in range(k) if j != i and j != (i + 1) % k])
        Q[i][j] = 0


def _more_zero_rate_categories(rng, md):
    """random_model draws a rate_mixture with a rate-0 category about once in forty models.  Here: half of the drawn
    rate_mixtures get one (and a prior that is not uniform), and one in eight of the models without any mixture gets a
    two- or three-category rate_mixture with one.  A category of positive rate and positive prior always remains."""
    mix = md.get("rate_mixture")
    if mix is None:
        if any(key.endswith("gamma_rate_mixture") for key in md) or rng.random() >= 0.125:
            return
        n = rng.randrange(2, 4)
        mix = md["rate_mixture"] = {"rates": [rng.choice([0.5, 1, 2.0]) for _ in range(n)], "prior": [1.0 / n] * n}
    elif rng.random() >= 0.5:
        return
    rates = mix["rates"]
    if len(rates) == 1:
        rates.append(rates[0] if rates[0] > 0 else 1.0)
    rates[rng.randrange(len(rates))] = 0
    if sum(rates) == 0:
        rates[rng.randrange(len(rates))] = rng.choice([0.5, 1, 2.0])
    w = [rng.random() + 0.1 for _ in rates]
    mix["prior"] = [v / sum(w) for v in w]


def _observe(rng, md):
    """latent states down the tree per site; every node missing, exact, or ambiguous with a positive entry at its latent
    state.  Returns the observation forms that occur."""
    edges, rates = md["edges"], md["edge_rate_coefficients"]
    k = len(md["rate_matrix"])
    n_nodes = len(edges) + 1
    coded = "character_data" in md
    S = len(md["character_data"] if coded else md["probability_array"])
    root, walk = top_down(edges)
    defs = md.get("character_definitions")
    seen = set()
    sites = []
    for _ in range(S):
        latent = [None] * n_nodes
        latent[root] = rng.randrange(k)
        for p, c, e in walk:
            latent[c] = latent[p] if rates[e] == 0 or rng.random() < 0.4 else rng.randrange(k)
        site = []
        for node in range(n_nodes):
            z = latent[node]
            r = rng.random()
            form = "missing" if r < 0.35 else "exact" if r < 0.7 else "ambiguous"
            if coded:
                if form == "ambiguous":
                    rows = [c for c in range(k + 1, len(defs)) if defs[c][z] > 0]
                    if rows:
                        site.append(rng.choice(rows))
                    else:
                        form = "exact"
                if form != "ambiguous":
                    site.append(k if form == "missing" else z)
            elif form == "missing":
                site.append([1] * k)
            elif form == "exact":
                site.append([1 if j == z else 0 for j in range(k)])
            else:
                row = [0 if rng.random() < 0.4 else round(rng.random(), 3) + 0.01 for _ in range(k)]
                if row[z] == 0:
                    row[z] = round(rng.random(), 3) + 0.01
                site.append(row)
            seen.add(form)
        sites.append(site)
    md["character_data" if coded else "probability_array"] = sites
    return seen


def _more_pair_listings(rng, x):
    """the trans axis beyond what random_query reaches: listings of more than four pairs (several passes of up to four
    directions at k = 4), duplicated pairs, and aggregated selections that hold a diagonal pair [i, i]"""
    k = len(x["model_and_data"]["rate_matrix"])
    r = rng.random()
    if r < 0.3:
        x["trans_reduction"] = {"selection": [[rng.randrange(k), rng.randrange(k)] for _ in range(rng.randrange(5, 10))]}
        return
    tr = x.get("trans_reduction")
    if r < 0.5:
        if tr is None or "selection" not in tr:
            tr = x["trans_reduction"] = {"selection": [[rng.randrange(k), rng.randrange(k)] for _ in range(rng.randrange(1, 4))]}
        at = rng.randrange(len(tr["selection"]) + 1)
        tr["selection"].insert(at, list(rng.choice(tr["selection"])))
        if isinstance(tr.get("aggregation"), list):
            tr["aggregation"].insert(at, round(rng.uniform(-1, 2), 3))
    elif r < 0.7:
        i = rng.randrange(k)
        pairs = [[rng.randrange(k), rng.randrange(k)] for _ in range(rng.randrange(1, 5))]
        pairs.insert(rng.randrange(len(pairs) + 1), [i, i])
        agg = rng.choice(["sum", "avg", "weights"])
        x["trans_reduction"] = {"selection": pairs,
                                "aggregation": agg if agg != "weights" else [round(rng.uniform(-1, 2), 3) for _ in pairs]}


def feasible_query(rng, kind):
    """(query, facts): a random_query draw with data of positive likelihood at every site; facts are what
    tests/test_expect_cases_cpu.py counts"""
    x = random_query(rng, kind)
    md = x["model_and_data"]
    _force_cycle(md)
    _more_structural_zeros(rng, md)
    _more_zero_rate_categories(rng, md)
    forms = _observe(rng, md)
    if kind == "trans":
        _more_pair_listings(rng, x)
    return x, facts(x, forms)


def facts(x, forms):
    md = x["model_and_data"]
    Q = md["rate_matrix"]
    k = len(Q)
    f = {"k": k, "edges": len(md["edges"]), "forms": forms,
         "zero_rate_edge": any(r == 0 for r in md["edge_rate_coefficients"]),
         "zero_in_Q": any(Q[i][j] == 0 for i in range(k) for j in range(k) if i != j),
         "zero_rate_category": (any(r == 0 for r in md.get("rate_mixture", {}).get("rates", []))
                                or md.get("gamma_rate_mixture", {}).get("invariable_prior", 0) > 0)}
    tr = x.get("trans_reduction") or {}
    sel = tr.get("selection")
    listed = sel is not None and "aggregation" not in tr
    f["many_listed_pairs_k4"] = k == 4 and listed and len(sel) > 4
    f["duplicate_pair"] = sel is not None and len({tuple(p) for p in sel}) < len(sel)
    f["aggregated_diagonal_pair"] = sel is not None and "aggregation" in tr and any(a == b for a, b in sel)
    agg = (x.get("state_reduction") or {}).get("aggregation")
    f["signed_state_weights"] = isinstance(agg, list) and min(agg) < 0 < max(agg)
    f["state_avg"] = agg == "avg"
    return f


_cases = {}


def cases(kind):
    """the NCASES seeded (query, facts) pairs of `kind`, the same objects for every caller"""
    if kind not in _cases:
        rng = random.Random(SEEDS[kind])
        _cases[kind] = [feasible_query(rng, kind) for _ in range(NCASES)]
    return _cases[kind]


def block(kind, b):
    return [x for x, _ in cases(kind)[b * BLOCK:(b + 1) * BLOCK]]


# ------------------------------------------------------------------ likelihood zero
_Q4 = [[0, 0.3, 0.4, 0.5], [0.3, 0, 0.3, 0.2], [0.1, 0.6, 0, 0.3], [0.7, 0.3, 0.2, 0]]
_BIRTH = [[0, 1, 0], [0, 0, 1], [0, 0, 0]]


def _infeasible():
    """(name, kind, query): site 1 of each document has likelihood zero, sites 0 and 2 do not.  Each cause once with
    site 1 the only selected site and once among several."""
    tree = {"edges": [[0, 1], [1, 2], [0, 3]], "edge_rate_coefficients": [0.3, 0.0, 0.2]}
    ok4 = [[1, 1, 1, 1], [0, 1, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1]]
    ok4b = [[0.5, 0.5, 0, 0], [1, 1, 1, 1], [0, 0, 1, 0], [1, 0, 0, 0]]
    ok3 = [[1, 0, 0], [1, 1, 1], [0, 0, 1], [0, 1, 0]]
    ok3b = [[1, 1, 1], [0, 1, 0], [0, 1, 0], [1, 1, 1]]
    causes = {
        # nodes 1 and 2 sit at the two ends of the rate-0 edge
        "zero_rate_edge": dict(tree, rate_matrix=_Q4, probability_array=[ok4, [[1, 1, 1, 1], [1, 0, 0, 0], [0, 0, 1, 0], [1, 1, 1, 1]], ok4b]),
        # every edge has a positive rate but all the prior sits on the rate-0 category
        "zero_rate_category": {"edges": tree["edges"], "edge_rate_coefficients": [0.3, 0.4, 0.2], "rate_matrix": _Q4,
                               "rate_mixture": {"rates": [0, 1.5], "prior": [1, 0]},
                               "probability_array": [[[1, 1, 1, 1], [0, 1, 0, 0], [0, 1, 0, 0], [0, 1, 0, 0]],
                                                     [[1, 1, 1, 1], [1, 0, 0, 0], [0, 0, 1, 0], [1, 1, 1, 1]],
                                                     [[0, 0, 1, 0], [1, 1, 1, 1], [0, 0, 1, 0], [1, 1, 1, 1]]]},
        # pure birth 0 -> 1 -> 2: node 1 in state 2 above node 2 in state 0
        "forbidden_transition": {"edges": tree["edges"], "edge_rate_coefficients": [0.3, 0.4, 0.2], "rate_matrix": _BIRTH,
                                 "probability_array": [ok3, [[1, 1, 1], [0, 0, 1], [1, 0, 0], [1, 1, 1]], ok3b]},
        "zero_root_row": {"edges": tree["edges"], "edge_rate_coefficients": [0.3, 0.4, 0.2], "rate_matrix": _Q4,
                          "root_prior": "uniform_distribution",
                          "probability_array": [ok4, [[0, 0, 0, 0], [0, 1, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1]], ok4b]},
    }
    kinds = {"zero_rate_edge": ("dwell", "em_update"), "zero_rate_category": ("trans", "dwell"),
             "forbidden_transition": ("em_update", "trans"), "zero_root_row": ("trans", "em_update")}
    out = []
    for name, md in causes.items():
        alone, among = kinds[name]
        for kind, tag, site_red in ((alone, "alone", {"selection": [1]}), (among, "among", {"selection": [2, 1, 0]})):
            q = {"model_and_data": copy.deepcopy(md), "site_reduction": dict(site_red)}
            if kind == "em_update":
                q["site_reduction"]["aggregation"] = "only" if tag == "alone" else "sum"
            elif kind == "trans":
                q["trans_reduction"] = {"selection": [[0, 1], [1, 2]]}
            out.append(("%s-%s-%s" % (name, tag, kind), kind, q))
    return out


INFEASIBLE = _infeasible()


def feasible_part(query):
    """the INFEASIBLE query with its site of likelihood zero left out of the selection"""
    q = copy.deepcopy(query)
    q["site_reduction"]["selection"] = [0, 2]
    if q["site_reduction"].get("aggregation") == "only":
        q["site_reduction"]["aggregation"] = "sum"
    return q


# ------------------------------------------------------------------ many copies of three patterns
DUPLICATE_FORM = {"dwell": "character_data", "trans": "probability_array", "em_update": "character_data"}
DUPLICATE_REDUCTIONS = (None, {"aggregation": "sum"}, {"selection": [5, 5, 17, 30, 2], "aggregation": [1.5, -0.5, 2, 1, 1]},
                        {"selection": [39, 0, 7, 7]})


def duplicate_sites_queries(kind):
    """the first case of `kind` in DUPLICATE_FORM[kind] with at least four edges whose first three sites differ, those
    three patterns repeated into 40 sites in a seeded order, under each site reduction the query takes (em-update:
    the aggregating ones).  Returns (order, [query, ...])."""
    form = DUPLICATE_FORM[kind]
    base = next(x for x, f in cases(kind) if form in x["model_and_data"] and f["edges"] >= 4
                and len({repr(p) for p in x["model_and_data"][form][:3]}) == 3)
    base = copy.deepcopy(base)
    md = base["model_and_data"]
    rng = random.Random(99)
    order = [rng.randrange(3) for _ in range(40)]
    assert set(order) == {0, 1, 2}
    pats = md[form][:3]
    md[form] = [pats[i] for i in order]
    out = []
    for red in DUPLICATE_REDUCTIONS:
        if kind == "em_update" and (red is None or "aggregation" not in red):
            continue
        y = {key: v for key, v in base.items() if key != "site_reduction"}
        if red is not None:
            y["site_reduction"] = copy.deepcopy(red)
        out.append(y)
    return order, out


# ------------------------------------------------------------------ known answers
def pure_birth_doc():
    """0 -> 1 -> 2 without return on a path of four edges, every node observed: the transitions happen on edges 0 and 2"""
    return {"model_and_data": {"edges": [[0, 1], [1, 2], [2, 3], [3, 4]], "edge_rate_coefficients": [1, 1, 2, 3], "rate_matrix": _BIRTH,
                               "probability_array": [[[1, 0, 0], [0, 1, 0], [0, 1, 0], [0, 0, 1], [0, 0, 1]]]}}


ABSORBING_RATES = [1, 1, 2, 0, 3]


def absorbing_doc(end_observed):
    """0 -> 1 without return on a path of five edges (one of rate 0), the root in state 0; the last node in state 1 or
    missing"""
    n = len(ABSORBING_RATES)
    rows = [[1, 0]] + [[1, 1]] * (n - 1) + [[0, 1] if end_observed else [1, 1]]
    return {"model_and_data": {"edges": [[i, i + 1] for i in range(n)], "edge_rate_coefficients": list(ABSORBING_RATES),
                               "rate_matrix": [[0, 1], [0, 0]], "probability_array": [rows]},
            "site_reduction": {"aggregation": "sum"}}


def algebra_doc():
    """seven edges, two sites, an asymmetric Q and one node with a fractional row"""
    return {"model_and_data": {
        "edges": [[5, 0], [5, 1], [5, 6], [6, 2], [6, 7], [7, 3], [7, 4]],
        "edge_rate_coefficients": [0.01, 0.2, 0.15, 0.3, 0.05, 0.3, 0.02],
        "rate_matrix": _Q4,
        "probability_array": [
            [[1, 0, 0, 0], [0, 1, 0, 0], [0, 1, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0.1, 0.2, 0.3, 0.4], [1, 1, 1, 1], [1, 1, 1, 1]],
            [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1], [0, 1, 0, 0], [0, 0, 1, 0], [0.1, 0.2, 0.3, 0.4], [1, 1, 1, 1], [1, 1, 1, 1]]]}}
