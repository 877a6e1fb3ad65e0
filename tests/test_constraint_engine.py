"""Constrained decoding at engine level: mg_generate_constrained through Engine.generate(constraint=) / generate_sampled(constraint=)
(include/mgrapher.h mg_constraint) on the tiny fixtures: greedy, beam search and sampled.  The emulator variants check LESS than the GPU
ones, because an emulated call takes seconds: one decode-step form (the device-counter form), one banned column, two images of the
per-image test, no sampled replay; the full versions run on the GPU.

  unconstrained()      the plain call: ids in both modes; token scores and top2 bit for bit against the plain call on the same (unfused)
                       selection tail, sampled with the same seed
  suppress             banning the token the plain answer holds at column j changes the answer from there on and never emits it
  one_of               every mode returns a candidate followed by EOS
  per-image semantics  row b of a constrained batch = the call on image b alone with its start state (cross-attention form pinned)
  replay               a second call of the same shape replays the captured step with the same bits; so does another automaton of the same
                       sizes, uploaded in place
  empty set            MG_E_INPUT after the call
"""
import numpy as np
import pytest

from markushgrapher_amd import constraint as K
from markushgrapher_amd.engine import MgError
from tests.test_decoder_prompt_engine import _case, _code, _modes
from tests.test_sampling_engine import _absorb_settings, _np, _same_ids

BACKENDS = [pytest.param("emu"), pytest.param("hip", marks=pytest.mark.gpu)]
FIXTURE = "g3_trained_tiny.npz"
SKW = dict(temperature=1.3, top_k=20, top_p=0.95, seed=41, return_scores=True)


def _forms(be_name):
    """decode-step forms: the emulator runs the device-counter form alone (what the captured graph replays; an emulated call takes seconds)"""
    return (2,) if be_name == "emu" else _modes(be_name)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _answers(ids, eos):
    """what each row wrote after the start token, up to (not including) its EOS; None for a row without EOS"""
    out = []
    for r in ids:
        e = np.flatnonzero(r[1:] == eos)
        out.append([int(t) for t in r[1:1 + e[0]]] if len(e) else None)
    return out


@pytest.mark.parametrize("be_name", BACKENDS)
def test_unconstrained_is_the_plain_call(be_name, monkeypatch):
    monkeypatch.setenv("MG_DECODE_FUSED_TAIL", "0")              # read when the engine is created: the plain call on the unfused tail
    eng, args, shape, _, T = _case(be_name, FIXTURE, T=12)
    monkeypatch.setenv("MG_DECODE_FUSED_TAIL", "1")
    fused, _, _, _, _ = _case(be_name, FIXTURE)
    free = K.unconstrained(shape.vocab_size, shape.eos_token_id)
    B = args[0].shape[0]
    for mode in _forms(be_name):
        eng.set_decode_graph(mode)
        fused.set_decode_graph(mode)
        try:
            a = eng.generate(*args, max_length=T, return_scores=True, return_top2=True)
            for e in ((eng,) if be_name == "emu" else (eng, fused)):      # (a constrained call runs the unfused tail whatever the engine's setting)
                b = e.generate(*args, max_length=T, return_scores=True, return_top2=True, constraint=free)
                assert np.array_equal(_np(e, b[0]), _np(eng, a[0]))
                assert np.array_equal(_bits(_np(e, b[3]["token_scores"])), _bits(_np(eng, a[3]["token_scores"])))
                ids, t2, t2p = _np(eng, a[0]), _np(e, b[2]), _np(eng, a[2])
                for r, row in enumerate(ids):                    # top2 of the columns a row wrote itself (a finished row sits in the sink:
                    n = 1 + len(_answers(row[None], shape.eos_token_id)[0] or row[1:-1]) + 1      # its top2 is the sink's, and nobody's)
                    assert np.array_equal(_bits(t2[1:n, r]), _bits(t2p[1:n, r])), (mode, r)
            f = fused.generate(*args, max_length=T)
            assert np.array_equal(_np(fused, f[0]), _np(eng, a[0]))                  # the fused plain call: the same ids
            for nr in (2,):
                kw = dict(max_length=T, num_return=nr, stream_ids=np.arange(B * nr) * 5 + 2, **SKW)
                s, q = eng.generate_sampled(*args, **kw), eng.generate_sampled(*args, constraint=free, **kw)
                assert np.array_equal(_np(eng, s[0]), _np(eng, q[0])) and np.array_equal(_bits(_np(eng, s[2])), _bits(_np(eng, q[2])))
        finally:
            eng.set_decode_graph(1)
            fused.set_decode_graph(1)


@pytest.mark.parametrize("be_name", BACKENDS)
def test_suppressed_token_changes_the_answer_from_its_column_on(be_name):
    """fails on a library without the constraint: the plain answer holds the token"""
    eng, args, shape, _, T = _case(be_name, FIXTURE)
    ids0 = _np(eng, eng.generate(*args, max_length=T)[0])
    V, eos, pad = shape.vocab_size, shape.eos_token_id, shape.pad_token_id
    tested = 0
    for j in ((1,) if be_name == "emu" else (1, 2, 3)):          # (an emulated call takes seconds)
        tok = int(ids0[0, j])
        if tok in (eos, pad):
            continue
        ids = _np(eng, eng.generate(*args, max_length=T, constraint=K.suppress(V, eos, [tok]))[0])
        assert not (ids[:, 1:] == tok).any()
        for b in range(ids0.shape[0]):
            at = np.flatnonzero(ids0[b, 1:] == tok)
            if len(at):                                          # the same up to the token's first column, another token there
                c = 1 + int(at[0])
                assert np.array_equal(ids[b, :c], ids0[b, :c]) and ids[b, c] != tok
            else:
                assert _same_ids(ids[b:b + 1], ids0[b:b + 1], pad)
        s = _np(eng, eng.generate_sampled(*args, max_length=T, constraint=K.suppress(V, eos, [tok]), **SKW)[0])
        assert not (s[:, 1:] == tok).any()
        tested += 1
    assert tested > 0


@pytest.mark.parametrize("be_name", BACKENDS)
def test_one_of_returns_a_candidate_followed_by_eos(be_name):
    eng, args, shape, _, T = _case(be_name, FIXTURE)
    V, eos, pad = shape.vocab_size, shape.eos_token_id, shape.pad_token_id
    ids0 = _np(eng, eng.generate(*args, max_length=T)[0])
    B = ids0.shape[0]
    own = [a for a in _answers(ids0, eos) if a]
    cands = [[11, 12, 13], [11, 40], [9]] + [a[:max(1, len(a) // 2)] + [21, 22] for a in own[:2]] + own[:1]
    cands = [c for c in cands if len(c) + 2 <= T and eos not in c and pad not in c]
    aut = K.one_of(V, eos, cands)
    g = _np(eng, eng.generate(*args, max_length=T, constraint=aut)[0])
    s = _np(eng, eng.generate_sampled(*args, max_length=T, num_return=2, constraint=aut, **SKW)[0])
    for out in (g, s):
        for a in _answers(out, eos):
            assert a is not None and a in cands, (a, cands)
    for b_, a in enumerate(_answers(ids0, eos)):                  # a plain answer among the candidates: every token of it is the row's
        if a in cands:                                            # arg-max and allowed, so greedy still writes it
            assert _answers(g, eos)[b_] == a


@pytest.mark.parametrize("be_name", BACKENDS)
def test_row_of_a_batch_is_the_call_on_its_image_alone(be_name):
    eng, args, shape, _, T = _case(be_name, FIXTURE, T=12)
    V, eos = shape.vocab_size, shape.eos_token_id
    ids0 = _np(eng, eng.generate(*args, max_length=T)[0])
    B = ids0.shape[0]
    words = [[int(ids0[0, 1])], [int(ids0[B - 1, 1]), int(ids0[B - 1, 2])], [30, 31]]
    words = [w for w in words if eos not in w]
    aut = K.bad_words(V, eos, words) & K.begin_suppress(V, eos, [int(ids0[0, 2]), 17])
    starts = np.array([aut.run(0, [30][:b % 2]) for b in range(B)], np.int32)      # ragged start states: image b has (not) seen token 30
    sid = np.arange(B) * 7 + 3
    skw = dict(max_length=T, min_length=T, temperature=1.3, top_k=20, top_p=0.95, seed=77)
    emu = be_name == "emu"                                       # (an emulated call takes seconds: one cross-attention form, two images)
    for absorb in _absorb_settings(eng)[:1 if emu else None]:
        eng.set_cross_absorb(absorb)
        try:
            g = _np(eng, eng.generate(*args, max_length=T, min_length=T, constraint=aut, constraint_start=starts)[0])
            s = _np(eng, eng.generate_sampled(*args, stream_ids=sid, constraint=aut, constraint_start=starts, **skw)[0])
            for b in ((1, B - 1) if emu else range(B)):
                one = tuple(a[b:b + 1] for a in args)
                g1 = eng.generate(*one, max_length=T, min_length=T, constraint=aut, constraint_start=starts[b:b + 1])[0]
                assert np.array_equal(_np(eng, g1), g[b:b + 1]), (absorb, "greedy", b)
                s1 = eng.generate_sampled(*one, stream_ids=sid[b:b + 1], constraint=aut, constraint_start=starts[b:b + 1], **skw)[0]
                assert np.array_equal(_np(eng, s1), s[b:b + 1]), (absorb, "sampled", b)
                for out in (g[b], s[b]):                          # and the rows obey the automaton from their start state
                    st = int(starts[b])
                    for t in out[1:]:
                        assert aut.allowed_mask(st)[t], (b, out)
                        st = aut.step(st, t)
        finally:
            eng.set_cross_absorb("auto")


@pytest.mark.parametrize("be_name", BACKENDS)
def test_second_call_replays_and_tables_are_refilled_in_place(be_name):
    eng, args, shape, _, T = _case(be_name, FIXTURE)
    V, eos, pad = shape.vocab_size, shape.eos_token_id, shape.pad_token_id
    ids0 = _np(eng, eng.generate(*args, max_length=T)[0])
    toks = [int(t) for t in ids0[0, 1:4] if t not in (eos, pad)][:2]
    assert len(toks) == 2 and toks[0] != toks[1]
    a, b = K.suppress(V, eos, [toks[0]]), K.suppress(V, eos, [toks[1]])
    assert (a.n_states, a.n_classes) == (b.n_states, b.n_classes)
    fresh = {}
    for name, aut in (("a", a), ("b", b)):                       # each automaton on an engine that has held no other
        e2, _, _, _, _ = _case(be_name, FIXTURE)
        r = e2.generate(*args, max_length=T, return_scores=True, constraint=aut)
        fresh[name] = (_np(e2, r[0]), _np(e2, r[3]["token_scores"]))
    order = (("a", a), ("b", b), ("a", a)) if be_name == "emu" else (("a", a), ("a", a), ("b", b), ("a", a), ("b", b))
    for mode in _forms(be_name):
        eng.set_decode_graph(mode)
        try:
            for name, aut in order:
                r = eng.generate(*args, max_length=T, return_scores=True, constraint=aut)
                assert np.array_equal(_np(eng, r[0]), fresh[name][0]), (mode, name)
                assert np.array_equal(_bits(_np(eng, r[3]["token_scores"])), _bits(fresh[name][1])), (mode, name)
                if mode == 1:
                    assert eng.decode_graph_active()
            if be_name == "emu":
                continue
            s1 = eng.generate_sampled(*args, max_length=T, constraint=a, **SKW)
            s2 = eng.generate_sampled(*args, max_length=T, constraint=a, **SKW)
            assert np.array_equal(_np(eng, s1[0]), _np(eng, s2[0])) and np.array_equal(_bits(_np(eng, s1[2])), _bits(_np(eng, s2[2])))
        finally:
            eng.set_decode_graph(1)
    assert not np.array_equal(fresh["a"][0], fresh["b"][0])


@pytest.mark.parametrize("be_name", BACKENDS)
def test_empty_allowed_set_and_validation(be_name):
    eng, args, shape, _, T = _case(be_name, FIXTURE, T=8)
    V, eos = shape.vocab_size, shape.eos_token_id
    B = args[0].shape[0]
    only_eos = K.one_of(V, eos, [[]])                             # the empty answer: the start state allows EOS only
    ids = _np(eng, eng.generate(*args, max_length=T, constraint=only_eos)[0])
    assert np.all(ids[:, 1] == eos)
    for call in (lambda: eng.generate(*args, max_length=T, min_length=3, constraint=only_eos),
                 lambda: eng.generate_sampled(*args, max_length=T, min_length=3, constraint=only_eos)):
        with pytest.raises(MgError) as e:                         # EOS-only below min_length: nothing is allowed
            call()
        assert _code(e) == -8 and "allows no token" in str(e.value)
    free = K.unconstrained(V, eos)
    for bad in (-1, free.n_states):
        st = np.zeros(B, np.int32)
        st[B - 1] = bad
        with pytest.raises(MgError) as e:
            eng.generate(*args, max_length=T, constraint=free, constraint_start=st)
        assert _code(e) == -2 and "start state" in str(e.value)
    with pytest.raises(ValueError):
        eng.generate(*args, max_length=T, constraint=K.unconstrained(V + 1, eos))
    with pytest.raises(ValueError):
        eng.generate(*args, max_length=T, constraint=free, constraint_start=[0])
    with pytest.raises(ValueError):
        eng.generate(*args, max_length=T, constraint_start=np.zeros(B, np.int32))
    with pytest.raises(TypeError):
        eng.generate_sampled(*args, max_length=T, constraint=lambda b, ids: [1])
    eng.debug_decode_capture(capture_steps=2, rows=B, forced_ids=np.zeros((B, T), np.int64))
    try:
        with pytest.raises(MgError) as e:
            eng.generate(*args, max_length=T, constraint=free)
        assert _code(e) == -5
    finally:
        eng.debug_decode_capture()
    eng.generate(*args, max_length=T, constraint=free)


# ---- beam search -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("be_name", BACKENDS)
def test_beam_unconstrained_is_the_plain_call(be_name):
    """ids, token scores, beam indices and sequences_scores bit for bit: the mask changes no candidate, the log-softmax is the plain one"""
    eng, args, shape, _, T = _case(be_name, FIXTURE, T=12)
    free = K.unconstrained(shape.vocab_size, shape.eos_token_id)
    for mode in _forms(be_name):
        eng.set_decode_graph(mode)
        try:
            kw = dict(num_beams=3, max_length=T, num_return=3, return_scores=True, length_penalty=0.7)
            a, b = eng.generate(*args, **kw), eng.generate(*args, constraint=free, **kw)
            for x, y in ((a[0], b[0]), (a[1], b[1]), (a[3]["token_scores"], b[3]["token_scores"]), (a[3]["beam_indices"], b[3]["beam_indices"])):
                x, y = _np(eng, x), _np(eng, y)
                assert x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), mode
            if mode == 1:
                assert eng.decode_graph_active()
        finally:
            eng.set_decode_graph(1)


@pytest.mark.parametrize("be_name", BACKENDS)
def test_beam_one_of_is_constrained_search_over_the_candidates(be_name):
    """beam-5 under one_of(five candidates): every returned hypothesis is a candidate followed by EOS, and the winner is the candidate that
    Engine.score_candidates ranks first.  length_penalty = 0: the score is the sum of the token log-probabilities, for which the early-stop
    heuristic is exact, and five beams hold every live prefix of five candidates - the search is exhaustive.  An image whose two best
    candidates are closer than the logit tolerance of the fixtures is left out; at most one may be."""
    from tests.test_scores import TOL
    eng, args, shape, _, T = _case(be_name, FIXTURE, T=12)
    V, eos, pad, start = shape.vocab_size, shape.eos_token_id, shape.pad_token_id, shape.decoder_start_token_id
    ids0 = _np(eng, eng.generate(*args, max_length=T)[0])
    B = ids0.shape[0]
    a0 = [t for t in (int(x) for x in ids0[0, 1:5]) if t not in (eos, pad)][:3]
    cands = [a0, a0[:1] + [33, 34], [35, 36, 37, 38], a0[:2] + [40], [41, 42]]
    assert len({tuple(c) for c in cands}) == 5
    aut = K.one_of(V, eos, cands)
    ids, sc, _, ex = eng.generate(*args, num_beams=5, max_length=T, num_return=3, length_penalty=0.0, return_scores=True, constraint=aut)
    ids, sc = _np(eng, ids), _np(eng, sc)
    answers = _answers(ids, eos)
    for r, a in enumerate(answers):
        if sc[r] > -1.0e8:                                        # (a finite hypothesis; fewer than num_return may exist)
            assert a in cands, (r, a)
    Tc = max(len(c) for c in cands) + 1
    tg = np.full((B, 5, Tc), -1, np.int64)
    dec = np.full((B, 5, Tc), pad, np.int64)
    for c, cand in enumerate(cands):
        full = cand + [eos]
        tg[:, c, :len(full)] = full
        dec[:, c, 0] = start
        dec[:, c, 1:len(full)] = full[:-1]
    tok = _np(eng, eng.score_candidates(*args, dec, tg)[0]).astype(np.float64)
    total = tok.sum(-1)                                           # [B, 5]; ignored targets score 0.0
    skipped = 0
    for b in range(B):
        order = np.argsort(-total[b])
        if total[b, order[0]] - total[b, order[1]] <= TOL:
            skipped += 1
            continue
        assert answers[b * 3] == cands[order[0]], (b, answers[b * 3], total[b])
        assert abs(sc[b * 3] - total[b, order[0]]) <= TOL
    assert skipped <= 1


@pytest.mark.parametrize("be_name", BACKENDS)
def test_beam_row_of_a_batch_and_replay(be_name):
    eng, args, shape, _, T = _case(be_name, FIXTURE, T=12)
    V, eos, pad = shape.vocab_size, shape.eos_token_id, shape.pad_token_id
    ids0 = _np(eng, eng.generate(*args, num_beams=3, max_length=T)[0])
    B = ids0.shape[0]
    aut = K.bad_words(V, eos, [[int(ids0[0, 1]), int(ids0[0, 2])], [30, 31]]) & K.begin_suppress(V, eos, [int(ids0[B - 1, 1])])
    starts = np.array([aut.run(0, [30][:b % 2]) for b in range(B)], np.int32)
    kw = dict(num_beams=3, max_length=T, return_scores=True, constraint=aut)
    bm = eng.generate(*args, constraint_start=starts, **kw)
    again = eng.generate(*args, constraint_start=starts, **kw)    # the second call of the shape replays the captured step
    assert np.array_equal(_np(eng, bm[0]), _np(eng, again[0])) and np.array_equal(_bits(_np(eng, bm[1])), _bits(_np(eng, again[1])))
    ids = _np(eng, bm[0])
    assert not np.array_equal(ids[:, :ids0.shape[1]], ids0[:, :ids.shape[1]])          # the automaton bites
    fill = pad or eos
    for b in ((1, B - 1) if be_name == "emu" else range(B)):
        one = tuple(a[b:b + 1] for a in args)
        b1 = eng.generate(*one, constraint_start=starts[b:b + 1], **kw)[0]
        assert _same_ids(_np(eng, b1), ids[b:b + 1], fill), b
        st = int(starts[b])
        for t in ids[b, 1:]:                                      # the best hypothesis obeys the automaton up to its EOS
            assert aut.allowed_mask(st)[t], (b, ids[b])
            st = aut.step(st, t)
            if t == eos:
                break
