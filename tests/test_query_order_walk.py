"""The walk of tests/test_gpu_query_order.py covers what that test says it covers (no GPU)."""
import pytest

from query_order_cases import covered, de_bruijn_pairs, held_covered, held_walk, walk


@pytest.mark.parametrize("n", [1, 2, 3, 10])
def test_every_ordered_pair_is_neighbours_once(n):
    seq = de_bruijn_pairs(n)
    assert len(seq) == n * n and set(seq) == set(range(n))
    pairs = [(seq[i], seq[(i + 1) % len(seq)]) for i in range(len(seq))]
    assert len(set(pairs)) == n * n
    assert set(pairs) == {(a, b) for a in range(n) for b in range(n)}


@pytest.mark.parametrize("n", [3, 10])
def test_two_walks_cover_every_triple(n):
    """|Q| = 10 is the GPU test's query count; 3 has an odd sequence length, so the state a query meets at a given place
    differs from one lap to the next, and the walk must not rely on an even one"""
    want = {(q1, s, q2) for q1 in range(n) for s in (0, 1) for q2 in range(n)}
    a, b = walk(n, 0), walk(n, 1)
    for steps, start in ((a, 0), (b, 1)):
        assert len(steps) == n * n + 1
        assert [s for _, s in steps] == [(start + i) % 2 for i in range(len(steps))]       # a change between every two queries
        assert len(covered(steps)) == n * n                                               # no pair twice within a walk
    assert covered(a) | covered(b) == want and len(want) == 2 * n * n
    assert covered(a) != want and covered(b) != want                                      # one walk alone does not
    # q2 always runs in the state q1 did not run in: "q1 at A, change, q2 at B" and the reverse
    for steps in (a, b):
        assert all(x[1] != y[1] for x, y in zip(steps, steps[1:]))


@pytest.mark.parametrize("n,full", [(10, (1, 2, 3, 9)), (3, (0, 2)), (4, (1, 3))])
def test_held_walk_shows_every_pair_right_after_a_change(n, full):
    """every ordered pair once as "change, q1, q2", in both states over the pairs; a state is held for two queries; every
    visit that does not begin with a full query follows a visit, in the other state, that holds one.  (10, four full
    queries) is the GPU test's walk."""
    for at in (0, 1):
        steps = held_walk(n, full, at)
        assert len(steps) == 2 * n * n
        got = held_covered(steps, at)
        assert len(got) == n * n and {(q1, q2) for q1, _, q2 in got} == {(x, y) for x in range(n) for y in range(n)}
        assert {s for _, s, _ in got} == {0, 1}
        visits = [(steps[i], steps[i + 1]) for i in range(0, len(steps), 2)]
        assert all(a[1] == b[1] for a, b in visits)
        assert all(v[0][1] != w[0][1] for v, w in zip(visits, visits[1:])) and visits[0][0][1] == 1 - at
        for prev, v in zip(visits, visits[1:]):
            if v[0][0] not in full:
                assert prev[0][0] in full or prev[1][0] in full
        assert visits[0][0][0] in full


def test_held_walk_refuses_what_it_cannot_order():
    with pytest.raises(ValueError):
        held_walk(3, (1,), 0)
