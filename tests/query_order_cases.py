"""The walk of tests/test_gpu_query_order.py (pure Python, no GPU): a cyclic order of n queries in which every ordered
pair of queries, a query followed by itself included, stands as neighbours exactly once (a de Bruijn sequence B(n, 2),
length n^2), run twice on an engine whose state alternates between two states A (0) and B (1) from one query to the
next: once starting in A, once starting in B.  tests/test_query_order_walk.py checks what is claimed for it: the two
walks together show every (query, state it ran in, next query) triple, 2 n^2 of them.

In those walks a change stands between every two queries, so the second query of a pair always finds the engine freshly
changed: what the first query of a pair leaves half done (transition matrices without their derivatives, a program
without its formats) is never what the second one starts from.  held_walk is the complement: the state changes before
every second query only, so that a pair runs as "change, q1, q2"; it shows every ordered pair so, once."""


def de_bruijn_pairs(n):
    """cyclic sequence over range(n) of length n * n: with L = n * n, the pairs (seq[i], seq[(i + 1) % L]) are all the
    n * n ordered pairs, each once (the Lyndon-word construction of B(n, 2))"""
    if n < 1:
        raise ValueError("at least one symbol")
    a = [0, 0, 0]
    seq = []

    def db(t, p):
        if t > 2:
            if 2 % p == 0:
                seq.extend(a[1:p + 1])
            return
        a[t] = a[t - p]
        db(t + 1, p)
        for j in range(a[t - p] + 1, n):
            a[t] = j
            db(t + 1, t)

    db(1, 1)
    return seq


def walk(n, start):
    """one walk: the sequence once round and its first query again, n * n + 1 steps (query, state); the state changes
    between every two consecutive steps, beginning with `start`"""
    seq = de_bruijn_pairs(n)
    return [(seq[i % len(seq)], (start + i) % 2) for i in range(len(seq) + 1)]


def covered(steps):
    """the (q1, state q1 ran in, q2) triples a walk shows: q2 is the query right after q1, in the other state"""
    return {(a[0], a[1], b[0]) for a, b in zip(steps, steps[1:])}


def held_walk(n, full, at):
    """every ordered pair of queries once as a visit "change, q1, q2" on an engine that is in state `at`: 2 n * n steps
    (query, state), the state changing before every visit and only there.

    With two states a stale buffer is seen only if its last writer ran in the other state.  `full` are the queries that
    leave nothing of the shared preparation undone; the visits are ordered so that every visit whose first query is not
    one of them directly follows a visit that holds one, which ran in the other state.  (A cyclic order run two queries
    to a visit does not do that: the Lyndon-word sequence reads 0 1 0 2 0 3 ..., visit after visit beginning alike.)
    Needs len(full) * n >= (n - len(full)) ** 2."""
    full = set(full)
    first = [(a, b) for a in range(n) if a in full for b in range(n)]
    second = [(a, b) for a in range(n) if a not in full for b in range(n) if b in full]
    neither = [(a, b) for a in range(n) if a not in full for b in range(n) if b not in full]
    if len(first) < len(neither) or (second and len(first) == len(neither)):
        raise ValueError("too few full queries to stand before every visit without one")
    visits = []
    for i, v in enumerate(neither):
        visits += [first[i], v]
    visits += first[len(neither):len(neither) + 1] + second + first[len(neither) + 1:]
    steps = []
    for q1, q2 in visits:
        at = 1 - at
        steps += [(q1, at), (q2, at)]
    return steps


def held_covered(steps, at):
    """the (q1, state, q2) triples a held walk shows as "change, q1, q2": q1 is the first query after a change, q2 runs
    right after it with no change in between (`at`: the state before the first step)"""
    out = set()
    for i in range(len(steps) - 1):
        before = steps[i - 1][1] if i else at
        if steps[i][1] != before and steps[i + 1][1] == steps[i][1]:
            out.add((steps[i][0], steps[i][1], steps[i + 1][0]))
    return out
