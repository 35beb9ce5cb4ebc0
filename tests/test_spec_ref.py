"""tests/spec_ref.py (the NumPy statement of the speculative-decoding rules the GPU tests compare
the kernels and generate(speculate=...) against) pinned on hand-worked cases. CPU only."""
import pytest

from spec_ref import accept, draft, simulate, totals


@pytest.mark.parametrize("tokens,held,k,ngram,feed,n", [
    # L = 1: nothing to look up; the k slots hold feed[0]
    ([5, 0, 0, 0, 0], 1, 3, 3, [5, 5, 5, 5], 0),
    # held out of range is clamped to [1, S]
    ([5, 0, 0, 0, 0], 0, 3, 3, [5, 5, 5, 5], 0),
    ([5, 0, 0, 0, 0], -7, 2, 8, [5, 5, 5], 0),
    ([1, 2, 3, 4], 100, 3, 3, [4, 4, 4, 4], 0),
    # no match at any g
    ([1, 2, 3, 4], 4, 3, 3, [4, 4, 4, 4], 0),
    # a match only at g = 1 (s = 0); the fourth draft is the first one again
    ([7, 1, 2, 7, 0, 0], 4, 3, 3, [7, 1, 2, 7], 3),
    ([7, 1, 2, 7, 0, 0], 4, 4, 3, [7, 1, 2, 7, 1], 4),
    # the rightmost of several matches: s = 2 (-> 8), not s = 0 (-> 9)
    ([3, 9, 3, 8, 3, 0, 0], 5, 3, 1, [3, 8, 3, 8], 3),
    # a longer g (s = 0, -> 5) wins over a nearer shorter one (g = 1 at s = 4, -> 6)
    ([1, 2, 5, 9, 2, 6, 1, 2, 0, 0], 8, 2, 2, [2, 5, 9], 2),
    ([1, 2, 5, 9, 2, 6, 1, 2, 0, 0], 8, 2, 1, [2, 6, 1], 2),
    # periodic extension: period 1, period 2, and a period above k (no self-extension needed)
    ([4, 4, 0, 0, 0], 2, 3, 3, [4, 4, 4, 4], 3),
    ([1, 2, 1, 2, 0, 0, 0], 4, 5, 3, [2, 1, 2, 1, 2, 1], 5),
    ([1, 2, 3, 4, 5, 6, 1, 2, 0, 0], 8, 3, 2, [2, 3, 4, 5], 3),
    # tokens past held are not part of the row
    ([1, 2, 3, 1, 2, 3], 3, 2, 3, [3, 3, 3], 0),
])
def test_draft_rule(tokens, held, k, ngram, feed, n):
    assert draft(tokens, held, k, ngram) == (feed, n)


def test_accept_rule():
    # a = 0..k
    for a in range(4):
        feed = [0, 5, 6, 7]
        c = [5, 6, 7, 8]
        if a < 3:
            feed[1 + a] = 99
        r = accept(c, feed, 3, count=2, held=10, limit=100)
        assert (r["a"], r["written"], r["count"], r["held"], r["done"], r["accepted"]) == \
            (a, c[:a + 1], 2 + a + 1, 10 + a + 1, False, a)
    # a padding slot past n_draft never counts, even when it matches
    r = accept([5, 5, 5, 5], [5, 5, 5, 5], 0, count=1, held=4, limit=100)
    assert (r["a"], r["written"], r["accepted"], r["drafted"]) == (0, [5], 0, 0)
    r = accept([5, 6, 7, 8], [0, 5, 6, 7], 1, count=1, held=4, limit=100)
    assert (r["a"], r["written"], r["accepted"], r["drafted"]) == (1, [5, 6], 1, 1)
    # eos inside the accepted run: written, stops the row there
    r = accept([5, 6, 7, 8], [0, 5, 6, 9], 3, count=3, held=9, limit=100, eos=6)
    assert (r["a"], r["written"], r["count"], r["held"], r["done"], r["accepted"]) == (2, [5, 6], 5, 11, True, 1)
    r = accept([5, 6, 7, 8], [0, 5, 6, 9], 3, count=3, held=9, limit=100, eos=5)
    assert (r["written"], r["done"], r["accepted"]) == ([5], True, 0)
    r = accept([5, 6, 7, 8], [0, 5, 6, 9], 3, count=3, held=9, limit=100, eos=7)  # the bonus token is the eos
    assert (r["written"], r["done"], r["accepted"]) == ([5, 6, 7], True, 2)
    # limit truncation
    r = accept([5, 6, 7, 8], [0, 5, 6, 7], 3, count=6, held=9, limit=8)
    assert (r["a"], r["written"], r["count"], r["done"], r["accepted"]) == (3, [5, 6], 8, True, 1)
    r = accept([5, 6, 7, 8], [0, 5, 6, 7], 3, count=7, held=9, limit=8)
    assert (r["written"], r["count"], r["done"], r["accepted"]) == ([5], 8, True, 0)


def test_simulate_on_a_loop():
    # prompt 1 2 3, plain ids 1 2 3 1 2 3 1 2 (limit 8), k = 2, ngram = 2, worked by hand:
    #   step 1: held 4, match g = 1 at s = 0 -> drafts 2 3, chosen 2 3 1: a = 2, three written
    #   step 2: held 7, match g = 2 at s = 2 -> drafts 2 3, chosen 2 3 1: a = 2, three written
    #   step 3: held 10, g = 2 at s = 5 -> drafts 2 3, chosen 2: a = 1 but one token to the limit
    r = simulate([1, 2, 3, 1, 2, 3, 1, 2], [1, 2, 3], 2, 2, 8)
    assert r["per_step"] == [(2, 2, 3), (2, 2, 3), (2, 1, 1)]
    assert (r["steps"], r["tokens"], r["drafted"], r["accepted"]) == (3, 8, 6, 4)
    # nothing ever matches: one token per step, nothing drafted
    r = simulate([4, 5, 6, 7], [1, 2, 3], 3, 3, 4)
    assert (r["steps"], r["tokens"], r["drafted"], r["accepted"]) == (3, 4, 0, 0)
    # stopped by an eos (plain returned 4 ids under a limit of 8): step 2 chooses the eos first
    r = simulate([1, 2, 3, 1], [1, 2, 3], 2, 2, 8, eos=9)
    assert r["per_step"] == [(2, 2, 3), (2, 0, 1)]
    assert (r["steps"], r["tokens"], r["drafted"], r["accepted"]) == (2, 5, 4, 2)
    # an eos inside the accepted run (it was drafted from the prompt): both drafts match, the
    # second is the eos, which is written and ends the row; one accepted draft was emitted
    r = simulate([1, 2], [1, 2, 3], 2, 2, 8, eos=3)
    assert r["per_step"] == [(2, 2, 2)]
    assert (r["steps"], r["tokens"], r["drafted"], r["accepted"]) == (1, 3, 2, 1)
    # the first token is the eos, or the limit is 1: no step
    assert simulate([], [1, 2], 2, 2, 8, eos=3)["steps"] == 0
    assert simulate([9], [1, 2], 2, 2, 1) == dict(steps=0, tokens=1, drafted=0, accepted=0, per_step=[])
    rows = [simulate([1, 2, 3, 1, 2, 3, 1, 2], [1, 2, 3], 2, 2, 8), simulate([4, 5, 6, 7], [1, 2, 3], 2, 3, 4)]
    assert totals(rows) == dict(steps=3, tokens=12, drafted=6, accepted=4)
