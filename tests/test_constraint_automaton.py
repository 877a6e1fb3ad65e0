"""markushgrapher_amd/constraint.py on the CPU: the builders against brute force on V = 37, the product, the constructor's refusals."""
import itertools

import numpy as np
import pytest

from markushgrapher_amd import constraint as K
from markushgrapher_amd.constraint import TokenAutomaton

V, EOS = 37, 2
# histories are drawn from a small alphabet that holds every token of the words / candidates, EOS apart, and one "other" token
ALPHA = [5, 6, 7, 8, 9, 20]
WORDS = [[5, 6], [6, 8, 9], [9], [7, 6, 8]]


def histories(alpha, max_len):
    for n in range(max_len + 1):
        yield from itertools.product(alpha, repeat=n)


def brute_bad_words(words, hist):
    """the tokens that complete no banned word after `hist` (stock NoBadWordsLogitsProcessor's rule)"""
    ok = np.ones(V, bool)
    for w in words:
        k = len(w) - 1
        if k == 0 or (len(hist) >= k and list(hist[len(hist) - k:]) == list(w[:-1])):
            ok[w[-1]] = False
    return np.nonzero(ok)[0]


def contains_word(words, hist):
    return any(list(hist[i:i + len(w)]) == list(w) for w in words for i in range(len(hist) - len(w) + 1))


@pytest.mark.parametrize("words", [WORDS, [[5, 6], [6, 7, 8], [6]], [[5, 6, 7], [6, 7], [7, 8, 9, 20], [20, 20]]], ids=["a", "b", "c"])
def test_bad_words_against_brute_force(words):
    """overlapping words: after every history of up to 5 tokens that holds no banned word, exactly the tokens that complete no banned word
    are allowed"""
    a = K.bad_words(V, EOS, words)
    assert a.n_classes == 2 + len({t for w in words for t in w})  # other, EOS, and the tokens of the words
    n = 0
    for h in histories(ALPHA, 5):
        if contains_word(words, h):
            continue
        s = a.run(0, h)
        assert s != a.sink
        assert np.array_equal(a.allowed(s), brute_bad_words(words, h)), h
        n += 1
    assert n > 500
    w = max(words, key=len)
    assert a.step(a.run(0, w[:-1]), w[-1]) == a.sink              # a disallowed token leads to the sink
    assert a.step(0, EOS) == a.sink and list(a.allowed(a.sink)) == [EOS]


def test_bad_words_single_tokens_is_the_one_state_case():
    a = K.bad_words(V, EOS, [[4], [11]])
    assert a.n_states == 2
    s = K.suppress(V, EOS, [4, 11])
    assert s.n_states == 2
    want = np.array([t for t in range(V) if t not in (4, 11)])
    assert np.array_equal(a.allowed(0), want) and np.array_equal(s.allowed(0), want)
    assert a.step(0, 20) == 0 and s.step(0, 20) == 0


def test_begin_suppress_two_states():
    a = K.begin_suppress(V, EOS, [4, EOS])
    assert a.n_states == 3
    assert np.array_equal(a.allowed(0), [t for t in range(V) if t not in (4, EOS)])
    assert a.step(0, 12) == 1 and np.array_equal(a.allowed(1), np.arange(V)) and a.step(1, 4) == 1 and a.step(1, EOS) == a.sink


def test_one_of_allows_exactly_the_continuations():
    cands = [[5, 6, 20], [5, 6], [5, 9, 9, 9], [20], [6, 5, 8, 7, EOS]]
    a = K.one_of(V, EOS, cands)
    cands = [c[:-1] if c[-1] == EOS else c for c in cands]
    seen_final = 0
    for h in histories(ALPHA, 5):
        h = list(h)
        if EOS in h:
            continue
        live = [c for c in cands if c[:len(h)] == h]
        want = sorted({c[len(h)] for c in live if len(c) > len(h)} | ({EOS} if h in cands else set()))
        if not live:
            assert a.run(0, h) == a.sink
            continue
        s = a.run(0, h)
        assert list(a.allowed(s)) == want, h
        if h in cands:
            assert a.step(s, EOS) == a.sink
            seen_final += 1
    assert seen_final == len(cands)


def test_product_is_the_intersection():
    a, b = K.bad_words(V, EOS, WORDS), K.one_of(V, EOS, [[5, 8, 6], [5, 6, 20], [20, 6, 8, 20], [8]])
    c, d = K.begin_suppress(V, EOS, [5, 20]), K.suppress(V, EOS, [8])
    for x, y in ((a, c), (a, d), (c, d), (b, K.unconstrained(V, EOS)), (K.bad_words(V, EOS, [[5, 6], [9]]), b)):
        p = x & y
        assert p.vocab == V and p.eos == EOS
        n = 0
        for h in histories(ALPHA, 4):
            sx = sy = sp = 0
            ok = True
            for t in h:                                           # histories that both allow, token by token
                if t not in x.allowed(sx) or t not in y.allowed(sy):
                    ok = False
                    break
                sx, sy, sp = x.step(sx, t), y.step(sy, t), p.step(sp, t)
            if not ok:
                continue
            assert np.array_equal(p.allowed(sp), np.intersect1d(x.allowed(sx), y.allowed(sy))), h
            n += 1
        assert n > 3
    # the classes are the common refinement: tokens share a class iff they share one in both
    p = a & c
    for t, u in itertools.combinations(range(V), 2):
        assert (p.cls[t] == p.cls[u]) == (a.cls[t] == a.cls[u] and c.cls[t] == c.cls[u])


def test_product_with_a_dead_pair_is_refused():
    """bad word [5] against the only candidate [5, 6]: the start state of the product allows nothing"""
    with pytest.raises(ValueError, match="allows no token"):
        K.bad_words(V, EOS, [[5]]) & K.one_of(V, EOS, [[5, 6]])


def test_constructor_refusals():
    cls = np.zeros(V, np.int64)
    cls[EOS] = 1
    ok = [[0, 1], [-1, 1]]
    TokenAutomaton(cls, ok, EOS)
    shared = cls.copy()
    shared[3] = 1                                                 # EOS shares its class with token 3
    with pytest.raises(ValueError, match="class of its own"):
        TokenAutomaton(shared, ok, EOS)
    with pytest.raises(ValueError, match="allows no token"):      # a dead state: state 1 allows nothing
        TokenAutomaton(cls, [[1, 2], [-1, -1], [-1, 2]], EOS)
    with pytest.raises(ValueError, match="allows no token"):      # state 1 allows class 2 only, which holds no token
        TokenAutomaton(cls, [[1, 2, -1], [-1, -1, 1], [-1, 2, -1]], EOS)
    with pytest.raises(ValueError, match="sink"):                 # the last state allows more than EOS
        TokenAutomaton(cls, [[0, 1], [1, 1]], EOS)
    with pytest.raises(ValueError, match="sink"):                 # ... or not even EOS
        TokenAutomaton(cls, [[0, 1], [-1, -1]], EOS)
    with pytest.raises(ValueError, match="outside"):
        TokenAutomaton(cls, [[0, 2], [-1, 1]], EOS)               # next state out of range
    with pytest.raises(ValueError, match="outside"):
        TokenAutomaton(cls + 1, ok, EOS)                          # class out of range
    with pytest.raises(ValueError, match="classes"):
        TokenAutomaton(cls, np.zeros((2, 4097), np.int64), EOS)
    with pytest.raises(ValueError, match="2\\*\\*24"):
        TokenAutomaton(cls, np.zeros((2 ** 13, 4096), np.int64), EOS)


def test_prefix_allowed_tokens_fn():
    a = K.one_of(V, EOS, [[5, 6], [9]])
    fn = a.as_prefix_allowed_tokens_fn()
    assert fn(0, np.array([0])) == [5, 9] and fn(0, [0, 5]) == [6] and fn(1, [0, 5, 6]) == [EOS]
    assert fn(0, [0, 5, 6, EOS]) == [EOS] and fn(0, [0, 20]) == [EOS]          # the sink
    s = a.run(0, [5])
    fn = a.as_prefix_allowed_tokens_fn(starts=[0, s], prompt_lens=[1, 3])
    assert fn(1, [0, 30, 5]) == [6] and fn(1, [0, 30, 5, 6]) == [EOS] and fn(0, [0]) == [5, 9]


def test_product_carries_the_forced_tables():
    """a prompt that holds a banned token: `suppress & bad_words` accepts it as its components do (stock does not look at a prompt), and the
    product's state after the prompt is the pair of the components' states"""
    a, b = K.suppress(V, EOS, [9]), K.bad_words(V, EOS, [[5, 6], [8]])
    p = a & b
    for prompt in ([9], [9, 5], [5, 6, 9, 5], [8, 8], [20, EOS, 5]):
        s = p.run_forced(0, prompt)
        assert s != p.sink, prompt
        assert np.array_equal(p.allowed(s), np.intersect1d(a.allowed(a.run_forced(0, prompt)), b.allowed(b.run_forced(0, prompt)))), prompt
    assert 6 not in p.allowed(p.run_forced(0, [9, 5])) and 6 in p.allowed(p.run_forced(0, [9]))
    q = K.one_of(V, EOS, [[5, 6]]) & a                            # a component without a forced table of its own keeps its default
    assert list(q.allowed(q.run_forced(0, [20]))) == [EOS] and list(q.allowed(q.run_forced(0, [5]))) == [6]
