"""constraint.one_of_each: one automaton holding a trie per image of a queue, against brute force on a 12-token vocabulary (CPU only)."""
import itertools

import numpy as np
import pytest

from markushgrapher_amd import constraint as K

V, EOS = 12, 1


def _accepted(aut, root, max_len=4):
    """every token sequence of up to max_len tokens (EOS excluded) that, followed by EOS, is accepted from `root` - by brute force over
    the vocabulary, through allowed_mask / step only"""
    out = set()
    toks = [t for t in range(V) if t != EOS]
    for n in range(max_len + 1):
        for seq in itertools.product(toks, repeat=n):
            s, ok = int(root), True
            for t in seq:
                if not aut.allowed_mask(s)[t]:
                    ok = False
                    break
                s = aut.step(s, t)
            if ok and aut.allowed_mask(s)[EOS] and aut.step(s, EOS) == aut.sink:
                out.add(seq)
    return out


LISTS = [
    [[2, 3], [2, 4], [5]],                 # shared prefix 2
    [[2, 3, 4]],                           # the same first tokens as image 0, another language
    [[5], [2, 4], [2, 3, EOS], [2, 3]],    # image 0's set again: order, a trailing EOS and a duplicate do not matter
    [[]],                                  # the empty candidate: EOS at once
    [[6, 6, 6], [6], []],                  # a candidate that is a prefix of another, and the empty one
    [[2, 3, 4]],                           # image 1's list
]


def test_accepted_language_per_root():
    aut, starts = K.one_of_each(V, EOS, LISTS)
    assert starts.shape == (len(LISTS),) and starts.dtype == np.int32
    for n, cands in enumerate(LISTS):
        want = set(tuple(t for t in c if t != EOS) for c in cands)
        assert _accepted(aut, starts[n]) == want, n
    # equal candidate sets share a root, different ones never do
    assert starts[0] == starts[2] and starts[1] == starts[5]
    assert len(set(starts.tolist())) == 4
    # conventions: "other" is class 0, EOS a class of its own, one class per distinct token, the sink last and EOS-only
    used = sorted({t for l in LISTS for c in l for t in c} | {EOS})
    assert aut.n_classes == len(used) + 1 and aut.cls[0] == 0 and aut.cls[11] == 0
    assert len(set(int(aut.cls[t]) for t in used)) == len(used) and all(aut.cls[t] > 0 for t in used)
    assert aut.allowed(aut.sink).tolist() == [EOS]
    # a trie per distinct set: states = nodes + sink (tries are NOT merged across images: image 1's [2, 3, 4] shares nothing with image 0's)
    nodes = 0
    for cands in (LISTS[0], LISTS[1], LISTS[3], LISTS[4]):
        pre = {()}
        for c in cands:
            c = [t for t in c if t != EOS]
            pre |= {tuple(c[:k]) for k in range(1, len(c) + 1)}
        nodes += len(pre)
    assert aut.n_states == nodes + 1


def test_one_image_is_one_of():
    """a queue of one image: the language of constraint.one_of"""
    cands = [[7, 8], [7, 9, 10], [3]]
    aut, starts = K.one_of_each(V, EOS, [cands])
    ref = K.one_of(V, EOS, cands)
    assert starts.tolist() == [0]
    assert _accepted(aut, 0) == _accepted(ref, 0) == {tuple(c) for c in cands}


def test_a_foreign_root_rejects_the_neighbours_answers():
    """what a leaked state would look like: image 1's root does not accept image 0's candidates"""
    aut, starts = K.one_of_each(V, EOS, LISTS)
    for c in LISTS[0]:
        s = aut.run(int(starts[1]), c)
        assert s == aut.sink or not aut.allowed_mask(s)[EOS], c
    assert not aut.allowed_mask(int(starts[1]))[5]
    assert aut.run(aut.sink, [2]) == aut.sink and _accepted(aut, aut.sink, 2) == {()}


def test_refusals():
    with pytest.raises(ValueError, match="image 1 has no candidate"):
        K.one_of_each(V, EOS, [[[2]], []])
    with pytest.raises(ValueError, match="EOS before its end"):
        K.one_of_each(V, EOS, [[[2, EOS, 3]]])
    with pytest.raises(ValueError, match="outside"):
        K.one_of_each(V, EOS, [[[2, V]]])
    with pytest.raises(ValueError, match="no images"):
        K.one_of_each(V, EOS, [])


def test_size_refusal_says_how_many_images_fit():
    """2^24 entries: images of one 300-token candidate over 310 distinct tokens = 301 nodes and at most 312 classes; 178 images fit
    (178 * 301 + 1 states x 312 classes = 16 716 648 <= 2^24 < 179 images'), so the 179th is refused by name.  4096 classes: the image that
    brings the distinct tokens (with EOS and "other") past 4096."""
    big_v = 5000
    rng = np.random.RandomState(0)
    pool = np.arange(2, 312)
    lists = [[[int(t) for t in rng.permutation(pool)[:300]]] for _ in range(200)]
    n_fit = 0
    while ((n_fit + 1) * 301 + 1) * 312 <= 1 << 24:
        n_fit += 1
    assert n_fit == 178
    with pytest.raises(ValueError, match=r"the first %d images fit" % n_fit):
        K.one_of_each(big_v, EOS, lists)
    aut, starts = K.one_of_each(big_v, EOS, lists[:n_fit])
    assert aut.n_states == n_fit * 301 + 1 and aut.n_states * aut.n_classes <= 1 << 24 and len(set(starts.tolist())) == n_fit
    wide = [[[2 + 1000 * n + j for j in range(1000)]] for n in range(5)]      # 1000 new tokens per image: 4 images = 4002 classes
    with pytest.raises(ValueError, match="the first 4 images fit"):
        K.one_of_each(big_v + 200, EOS, wide)
    assert K.one_of_each(big_v + 200, EOS, wide[:4])[0].n_classes == 4002
