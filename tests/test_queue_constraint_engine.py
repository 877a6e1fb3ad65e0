"""Decoder prompt and constraint in the greedy, sampled and beam queues (C ABI mg_generate_stream_constrained /
mg_generate_stream_beam_constrained through Engine.generate_stream / generate_stream_sampled / generate_stream_beam).  Prompt and start
state are per IMAGE of the queue; a slot that is handed the next image takes that image's first prompt token and start state.  Every test is
an EQUALITY with code from before the queue forms took these: one-image batch calls (Engine.generate, Engine.generate_sampled with the
sequence's stream id) or the plain queue.  `emu` = the same sources on the CPU SIMT emulator, `hip` = MI355X (the step is a captured graph).

Rig: g3_trained_tiny.npz (6 images, golden greedy answers of 3 .. 10 tokens, images 0 and 1 share one), T = 16, the queue ORDER of 14
entries, geometries (chunk, slots, pool_chunks) = (4, 3, 2), (3, 5, 3), (6, 2, 2): every slot is handed over, no chunk divides the queue, pool
entries are recycled under live images.  An emulated beam-5 queue call takes tens of seconds, so the emulator variants run the first
geometry, the K / V cross-attention form and the first 7 queue entries (every slot of the three is still handed over); the hip variants run
all three geometries, both forms and all 14 entries.

  null identities     [start]-only prompts, unconstrained() and both = the plain queue (ids, lengths, score bits), three modes
  self-prefix         a prompt that is a prefix of the plain queue's row reproduces it; forced columns score 0.0
  suppress            rows = one-image batch calls, three modes
  one_of_each         a trie per entry: slot hand-over resets the state; rows = one-image batch calls; beam-5 with num_return 2
  empty set           MG_E_INPUT after a complete call; the row is [start, eos]; its slot is freed
  replay and key      same shape replays; tables refilled in place; n_states / ld / pointer changes; plain calls interleaved
  validation          each bad argument names itself
"""
import numpy as np
import pytest

from markushgrapher_amd import constraint as K
from markushgrapher_amd.engine import MgError
from tests.test_sampling_stream import BACKENDS, ORDER, SEED, TEMP, _absorb_settings, _args, _case, _np

T = 16
GEOS = ((4, 3, 2), (3, 5, 3), (6, 2, 2))
SUPPRESSED = (208, 478, 270, 331)      # the tokens the golden answers hold at column 2
SKW = dict(temperature=TEMP, top_k=0, top_p=1.0, seed=SEED)
NB = 5


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _geos(be_name):
    return GEOS[:1] if be_name == "emu" else GEOS


def _order(be_name):
    return ORDER[:7] if be_name == "emu" else ORDER


def _min_handovers(order, slots=3):
    return min(2, (len(order) - slots) // slots)


def _forms(be_name, eng):
    return [False] if be_name == "emu" else _absorb_settings(eng)


def _answers(g, eos):
    """the golden greedy answers without start token and EOS"""
    out = []
    for row in g["greedy_ids"]:
        e = np.flatnonzero(row == eos)
        out.append([int(t) for t in row[1:int(e[0])]])
    return out


def _handovers(lens, slots):
    """hand-overs per slot under slot_refill's rule (idle slots take the next sequences in slot order), every image ready: a model of the
    schedule, for the non-vacuity counts only"""
    busy, count, head = [0] * slots, [-1] * slots, 0
    while head < len(lens):
        for r in range(slots):
            if busy[r] == 0 and head < len(lens):
                busy[r] = int(lens[head]) - 1
                count[r] += 1
                head += 1
        step = min(b for b in busy if b > 0)
        busy = [max(0, b - step) for b in busy]
    return count


def _cut(ids, plen, eos, cols):
    e = np.flatnonzero(ids[plen:] == eos)
    return int(e[0]) + plen + 1 if len(e) else cols


def _one_greedy(eng, inp, b, shape, prompt=None, plen=1, **kw):
    """Engine.generate on image b alone -> (ids cut at the length, token scores)"""
    pk = {} if prompt is None else dict(decoder_prompt=prompt[None, :], decoder_prompt_len=[plen])
    ids, _, _, ex = eng.generate(*_args(inp, [b]), max_length=T, return_scores=True, **pk, **kw)
    ids, ts = _np(eng, ids)[0], _np(eng, ex["token_scores"])[0]
    n = _cut(ids, plen, shape.eos_token_id, len(ids))
    return ids[:n], ts[:n - 1]


def _one_sampled(eng, inp, b, q, shape, prompt=None, plen=1, **kw):
    pk = {} if prompt is None else dict(decoder_prompt=prompt[None, :], decoder_prompt_len=[plen])
    ids, cols, ts = eng.generate_sampled(*_args(inp, [b]), stream_ids=[q], return_scores=True, max_length=T, **SKW, **pk, **kw)
    ids, ts = _np(eng, ids)[0], _np(eng, ts)[0]
    n = _cut(ids, plen, shape.eos_token_id, len(ids))
    return ids[:n], ts[:n - 1]


def _one_beam(eng, inp, b, prompt=None, plen=1, nr=2, **kw):
    pk = {} if prompt is None else dict(decoder_prompt=prompt[None, :], decoder_prompt_len=[plen])
    ids, sc, _, ex = eng.generate(*_args(inp, [b]), num_beams=NB, num_return=nr, max_length=T, return_scores=True, **pk, **kw)
    return _np(eng, ids), _np(eng, sc), _np(eng, ex["token_scores"]), _np(eng, ex["beam_indices"])


def _check_greedy_rows(eng, r, want, shape, what):
    ids, lens, ts = _np(eng, r[0]), _np(eng, r[1]), _np(eng, r[3])
    for q, (row, sc) in enumerate(want):
        n = len(row)
        assert lens[q] == n, (what, q, lens[q], n)
        assert np.array_equal(ids[q, :n], row), (what, q, ids[q].tolist(), row.tolist())
        assert np.all(ids[q, n:] == shape.pad_token_id), (what, q)
        assert np.array_equal(_bits(ts[q, :n - 1]), _bits(sc)), (what, q)
        assert np.all(ts[q, n - 1:] == 0.0), (what, q)


def _check_beam_rows(eng, r, want, nr, what):
    """r = generate_stream_beam(num_return=nr, return_scores=True); want[q] = the one-image call's (ids [nr, cols], scores, token scores,
    beam indices numbered from row 0)"""
    ids, lens, sc, ex = _np(eng, r[0]), _np(eng, r[1]), _np(eng, r[2]), r[4]
    ts, bi = _np(eng, ex["token_scores"]), _np(eng, ex["beam_indices"])
    for q, (wi, ws, wt, wb) in enumerate(want):
        rows, n = slice(q * nr, (q + 1) * nr), wi.shape[1]
        assert lens[q] == n, (what, q, lens[q], n)
        assert np.array_equal(ids[rows, :n], wi), (what, q, ids[rows].tolist(), wi.tolist())
        assert np.array_equal(_bits(sc[rows]), _bits(ws)), (what, q)
        assert np.array_equal(_bits(ts[rows, :n - 1]), _bits(wt)), (what, q)
        assert np.array_equal(bi[rows, :n - 1], np.where(wb >= 0, wb + q * NB, wb)), (what, q)


def _start_prompts(n, shape):
    return np.full((n, 1), shape.decoder_start_token_id, np.int64)


@pytest.mark.parametrize("be_name", BACKENDS)
def test_null_identities_give_the_plain_queue(be_name):
    """A prompt of [start] alone, unconstrained(), and both: ids, lengths and token-score bits of the plain queue in the greedy and the
    sampled queue; the beam queue's n-best ids, lengths, sequence scores, token scores and beam indices.  (None for both takes the plain
    entry point: the Python layer does not reach the new one.)"""
    eng, inp, shape, _, g = _case(be_name)
    ORDER = _order(be_name)
    q = _args(inp, ORDER)
    free = K.unconstrained(shape.vocab_size, shape.eos_token_id)
    variants = (dict(decoder_prompt=_start_prompts(len(ORDER), shape)), dict(constraint=free),
                dict(decoder_prompt=_start_prompts(len(ORDER), shape), constraint=free))
    for absorb in _forms(be_name, eng):
        eng.set_cross_absorb(absorb)
        try:
            for chunk, slots, pool_chunks in _geos(be_name):
                geo = dict(max_length=T, chunk=chunk, slots=slots, pool_chunks=pool_chunks)
                for call, kw in ((eng.generate_stream, {}), (eng.generate_stream_sampled, SKW)):
                    ref = call(*q, return_scores=True, **kw, **geo)
                    assert len(set(_np(eng, ref[1]).tolist())) > 1
                    # (emulator: the sampled and the beam queue check prompt and automaton together only)
                    for v in (variants[2:] if be_name == "emu" and kw else variants):
                        r = call(*q, return_scores=True, **kw, **v, **geo)
                        assert np.array_equal(_np(eng, r[0]), _np(eng, ref[0])), (call.__name__, list(v))
                        assert np.array_equal(_np(eng, r[1]), _np(eng, ref[1])), (call.__name__, list(v))
                        assert np.array_equal(_bits(_np(eng, r[3])), _bits(_np(eng, ref[3]))), (call.__name__, list(v))
                # NULL for samp, prompt and constraint through the new entry point itself: the greedy queue's call
                import ctypes as C
                ref = eng.generate_stream(*q, **geo)
                ids, bb, am, pv, N, L = eng._inputs(*q)
                out, ln = eng.mem.empty((N, T), np.int64), eng.mem.empty((N,), np.int32)
                rc = eng.lib.mg_generate_stream_constrained(eng.model, eng.mem.stream(), eng.mem.ptr(eng._sws), eng._sws_bytes, eng.mem.ptr(ids),
                                                            eng.mem.ptr(bb), eng.mem.ptr(am), eng.mem.ptr(pv), N, L, chunk, slots, pool_chunks, T, 0,
                                                            eng.mem.ptr(out), eng.mem.ptr(ln), None, None, None, None, None)
                assert rc == 0 and np.array_equal(_np(eng, out), _np(eng, ref[0])) and np.array_equal(_np(eng, ln), _np(eng, ref[1]))
                bgeo = dict(geo, slots=min(slots, 3), num_beams=NB, num_return=2, return_scores=True)
                ref = eng.generate_stream_beam(*q, **bgeo)
                for v in (variants[2:] if be_name == "emu" else variants):
                    r = eng.generate_stream_beam(*q, **v, **bgeo)
                    for i in (0, 1, 2):
                        assert np.array_equal(_bits(_np(eng, r[i])) if i == 2 else _np(eng, r[i]), _bits(_np(eng, ref[i])) if i == 2 else _np(eng, ref[i])), (i, list(v))
                    assert np.array_equal(_bits(_np(eng, r[4]["token_scores"])), _bits(_np(eng, ref[4]["token_scores"]))), list(v)
                    assert np.array_equal(_np(eng, r[4]["beam_indices"]), _np(eng, ref[4]["beam_indices"])), list(v)
        finally:
            eng.set_cross_absorb("auto")


@pytest.mark.parametrize("be_name", BACKENDS)
def test_self_prefix_reproduces_the_plain_queue(be_name):
    """Entry n is prompted with [start] + the first n % 3 tokens of what the plain queue writes for it (greedy: its golden answer; 3 is
    the shortest answer, so every prompt leaves a free column.  Sampled: the plain sampled queue's row, cut so that one free column is
    left).  ids, lengths and the free columns' score bits are the plain queue's, the forced columns score 0.0.  Non-vacuity: at least
    half of the entries carry a prompt longer than [start] (9 of 14 greedy), of two different lengths."""
    eng, inp, shape, _, g = _case(be_name)
    ORDER = _order(be_name)
    q = _args(inp, ORDER)
    N = len(ORDER)
    for absorb in _forms(be_name, eng):
        eng.set_cross_absorb(absorb)
        try:
            for chunk, slots, pool_chunks in _geos(be_name):
                geo = dict(max_length=T, chunk=chunk, slots=slots, pool_chunks=pool_chunks)
                for call, kw in ((eng.generate_stream, {}), (eng.generate_stream_sampled, SKW)):
                    ref = call(*q, return_scores=True, **kw, **geo)
                    ri, rl, rt = _np(eng, ref[0]), _np(eng, ref[1]), _np(eng, ref[3])
                    if call == eng.generate_stream:
                        for n, b in enumerate(ORDER):
                            assert np.array_equal(ri[n, :rl[n]], g["greedy_ids"][b][:rl[n]]), n
                    lens = np.array([1 + min(n % 3, rl[n] - 3) for n in range(N)], np.int32)
                    assert lens.min() >= 1 and int((lens > 1).sum()) >= N // 2 and len(set(lens.tolist())) == 3
                    prompt = np.full((N, 3), shape.decoder_start_token_id, np.int64)
                    for n in range(N):
                        prompt[n, :lens[n]] = ri[n, :lens[n]]
                    r = call(*q, return_scores=True, decoder_prompt=prompt, decoder_prompt_len=lens, **kw, **geo)
                    assert np.array_equal(_np(eng, r[0]), ri) and np.array_equal(_np(eng, r[1]), rl), call.__name__
                    ts = _np(eng, r[3])
                    for n in range(N):
                        assert np.all(ts[n, :lens[n] - 1] == 0.0), (call.__name__, n)
                        assert np.array_equal(_bits(ts[n, lens[n] - 1:]), _bits(rt[n, lens[n] - 1:])), (call.__name__, n)
        finally:
            eng.set_cross_absorb("auto")


@pytest.mark.parametrize("be_name", BACKENDS)
def test_suppress_rows_equal_one_image_calls(be_name):
    """suppress_tokens {208, 478, 270, 331} - the golden answers' tokens at column 2 - in the greedy, the sampled (temperature 1.5, seed
    20261, stream id = the place in the queue) and the beam-5 queue (num_return 2): sequence q = the batch call on its image alone.
    Non-vacuity, measured on the one-image greedy reference calls (full queue; the same on the emulator and the GPU, both forms): 14 of
    14 rows differ from their golden answer, all at column 2, none holds a suppressed token, lengths {4, 5, 6, 8, 12, 16}; on 3 slots the
    slots are handed over 4, 4 and 3 times.  First 7 entries (the emulator variant): 7 of 7, six distinct lengths, every slot handed over."""
    eng, inp, shape, _, g = _case(be_name)
    ORDER = _order(be_name)
    q = _args(inp, ORDER)
    V, eos = shape.vocab_size, shape.eos_token_id
    sup = K.suppress(V, eos, SUPPRESSED)
    for absorb in _forms(be_name, eng):
        eng.set_cross_absorb(absorb)
        try:
            want = [_one_greedy(eng, inp, b, shape, constraint=sup) for b in ORDER]
            differ = sum(1 for n, b in enumerate(ORDER) if not np.array_equal(want[n][0], g["greedy_ids"][b][:len(want[n][0])]))
            lens = [len(w[0]) for w in want]
            print(f"absorb {absorb}: {differ} of {len(ORDER)} rows differ from golden, lengths {sorted(set(lens))}, hand-overs {_handovers(lens, 3)}")
            assert differ == len(ORDER) and len(set(lens)) >= 4
            assert all(w[0][2] != g["greedy_ids"][b][2] and not set(w[0].tolist()) & set(SUPPRESSED) for w, b in zip(want, ORDER))
            assert min(_handovers(lens, 3)) >= _min_handovers(ORDER)
            want_s = [_one_sampled(eng, inp, b, n, shape, constraint=sup) for n, b in enumerate(ORDER)]
            assert not any(set(w[0].tolist()) & set(SUPPRESSED) for w in want_s) and len(set(len(w[0]) for w in want_s)) > 1
            want_b = [_one_beam(eng, inp, b, constraint=sup) for b in ORDER]
            for chunk, slots, pool_chunks in _geos(be_name):
                geo = dict(max_length=T, chunk=chunk, slots=slots, pool_chunks=pool_chunks)
                _check_greedy_rows(eng, eng.generate_stream(*q, return_scores=True, constraint=sup, **geo), want, shape, ("greedy", geo))
                _check_greedy_rows(eng, eng.generate_stream_sampled(*q, return_scores=True, constraint=sup, **SKW, **geo), want_s, shape,
                                   ("sampled", geo))
                r = eng.generate_stream_beam(*q, num_beams=NB, num_return=2, return_scores=True, constraint=sup, **dict(geo, slots=min(slots, 3)))
                _check_beam_rows(eng, r, want_b, 2, ("beam", geo))
        finally:
            eng.set_cross_absorb("auto")


def _tries(shape, g, ORDER):
    """one_of_each for the queue: the entry with image b may answer with the golden answer of image (b + 2) % 6 or (b + 3) % 6 - never its
    own (images 0 and 1 share an answer: 0 gets {2, 3}, 1 gets {3, 4}), and neighbours in ORDER have different tries.  Entries with
    n % 3 == 1 are prompted with [start, first token of the first candidate]."""
    V, eos, start = shape.vocab_size, shape.eos_token_id, shape.decoder_start_token_id
    ans = _answers(g, eos)
    cands = [[ans[(b + 2) % 6], ans[(b + 3) % 6]] for b in ORDER]
    aut, roots = K.one_of_each(V, eos, cands)
    prompt = np.full((len(ORDER), 2), start, np.int64)
    lens = np.ones(len(ORDER), np.int32)
    for n in range(len(ORDER)):
        if n % 3 == 1:
            prompt[n, 1], lens[n] = cands[n][0][0], 2
    starts = np.array([aut.run_forced(int(roots[n]), prompt[n, 1:lens[n]]) for n in range(len(ORDER))], np.int32)
    return aut, cands, prompt, lens, starts


@pytest.mark.parametrize("be_name", BACKENDS)
def test_one_of_each_across_slot_hand_over(be_name):
    """Every output is one of ITS entry's candidates followed by EOS and equals the one-image call with that entry's prompt and start
    state.  A state that leaked across a hand-over would leave the new sequence in the previous one's sink (EOS only) or in a foreign trie:
    both assertions fail.  Greedy, sampled, and beam-5 with num_return 2 (hypotheses, scores, token scores, beam indices).
    Non-vacuity (one-image greedy references, full queue; the same on the emulator and the GPU, both forms): 14 of 14 rows differ from
    their golden answer, lengths {5, 6, 8, 10, 11}, the first and the second candidate of a list are both chosen somewhere, 5 entries carry
    a two-token prompt; on 3 slots the slots are handed over 4, 3 and 4 times."""
    eng, inp, shape, _, g = _case(be_name)
    ORDER = _order(be_name)
    q = _args(inp, ORDER)
    eos = shape.eos_token_id
    aut, cands, prompt, lens, starts = _tries(shape, g, ORDER)
    pkw = dict(decoder_prompt=prompt, decoder_prompt_len=lens, constraint=aut, constraint_start=starts)

    def one(n):
        return dict(prompt=prompt[n], plen=int(lens[n]), constraint=aut, constraint_start=[int(starts[n])])

    def is_candidate(n, row):
        return row[-1] == eos and [int(t) for t in row[1:-1]] in cands[n]

    for absorb in _forms(be_name, eng):
        eng.set_cross_absorb(absorb)
        try:
            want = [_one_greedy(eng, inp, b, shape, **one(n)) for n, b in enumerate(ORDER)]
            wl = [len(w[0]) for w in want]
            differ = sum(1 for n, b in enumerate(ORDER) if not np.array_equal(want[n][0], g["greedy_ids"][b][:wl[n]]))
            which = set(cands[n].index([int(t) for t in w[0][1:-1]]) for n, w in enumerate(want))
            print(f"absorb {absorb}: {differ} of {len(ORDER)} differ from golden, lengths {sorted(set(wl))}, candidate indices chosen {which}, "
                  f"hand-overs {_handovers(wl, 3)}")
            assert differ == len(ORDER) and len(set(wl)) >= 3 and int((lens == 2).sum()) == len(range(1, len(ORDER), 3))
            assert all(is_candidate(n, w[0]) for n, w in enumerate(want))
            assert min(_handovers(wl, 3)) >= _min_handovers(ORDER)
            want_s = [_one_sampled(eng, inp, b, n, shape, **one(n)) for n, b in enumerate(ORDER)]
            want_b = [_one_beam(eng, inp, b, **one(n)) for n, b in enumerate(ORDER)]
            for chunk, slots, pool_chunks in _geos(be_name):
                geo = dict(max_length=T, chunk=chunk, slots=slots, pool_chunks=pool_chunks)
                for what, call, kw, w in (("greedy", eng.generate_stream, {}, want), ("sampled", eng.generate_stream_sampled, SKW, want_s)):
                    r = call(*q, return_scores=True, **kw, **pkw, **geo)
                    ids, ln = _np(eng, r[0]), _np(eng, r[1])
                    assert all(is_candidate(n, ids[n, :ln[n]]) for n in range(len(ORDER))), (what, geo, ids.tolist())
                    _check_greedy_rows(eng, r, w, shape, (what, geo))
                r = eng.generate_stream_beam(*q, num_beams=NB, num_return=2, return_scores=True, **pkw, **dict(geo, slots=min(slots, 3)))
                ids = _np(eng, r[0])
                for n in range(len(ORDER)):      # the best hypothesis is a candidate (the second may be an unfinished beam's tail)
                    e = np.flatnonzero(ids[2 * n, 1:] == eos)
                    assert len(e) and is_candidate(n, ids[2 * n, :int(e[0]) + 2]), (n, ids[2 * n].tolist())
                _check_beam_rows(eng, r, want_b, 2, ("beam", geo))
        finally:
            eng.set_cross_absorb("auto")


@pytest.mark.parametrize("be_name", BACKENDS)
def test_empty_allowed_set_frees_the_slot(be_name):
    """Entry 4 starts in the sink (EOS only) with min_length 3: the call completes, returns MG_E_INPUT, that sequence is [start, eos] with
    score 0.0, every other sequence equals its one-image call (the slot was freed and handed on: 14 sequences on 3 slots all finish), and
    the engine works afterwards.  Greedy and sampled; beam search has no empty-set rule."""
    eng, inp, shape, _, g = _case(be_name)
    ORDER = _order(be_name)
    eng.set_cross_absorb(False)
    try:
        q = _args(inp, ORDER)
        V, eos, start = shape.vocab_size, shape.eos_token_id, shape.decoder_start_token_id
        free = K.unconstrained(V, eos)
        starts = np.zeros(len(ORDER), np.int32)
        starts[4] = free.sink
        geo = dict(max_length=T, min_length=3, chunk=4, slots=3, pool_chunks=2)
        plain = eng.generate_stream(*q, **geo)
        for what, call, kw in (("greedy", eng.generate_stream, {}), ("sampled", eng.generate_stream_sampled, SKW)):
            with pytest.raises(MgError) as e:
                call(*q, return_scores=True, constraint=free, constraint_start=starts, **kw, **geo)
            assert "error -8" in str(e.value) and "allows no token" in str(e.value) and "1 sequences" in str(e.value), what
            r = e.value.outputs
            ids, lens, ts = _np(eng, r[0]), _np(eng, r[1]), _np(eng, r[3])
            assert lens[4] == 2 and ids[4, :2].tolist() == [start, eos] and np.all(ids[4, 2:] == shape.pad_token_id) and np.all(ts[4] == 0.0), what
            for n, b in enumerate(ORDER):
                if n == 4:
                    continue
                one = _one_greedy if what == "greedy" else (lambda *a, **k: _one_sampled(*a[:3], n, *a[3:], **k))
                row, sc = one(eng, inp, b, shape, constraint=free, min_length=3)
                assert lens[n] == len(row) and np.array_equal(ids[n, :len(row)], row) and np.array_equal(_bits(ts[n, :len(row) - 1]), _bits(sc)), (what, n)
        again = eng.generate_stream(*q, **geo)
        assert np.array_equal(_np(eng, again[0]), _np(eng, plain[0])) and np.array_equal(_np(eng, again[1]), _np(eng, plain[1]))
    finally:
        eng.set_cross_absorb("auto")


@pytest.mark.parametrize("be_name", BACKENDS)
def test_replay_and_step_key(be_name):
    """Back-to-back calls on one engine (hip: the captured queue step is replayed or re-captured by its key; the emulator runs the same
    sequence eagerly).  Same shape: same bits, the graph is active.  Another automaton of the same sizes is uploaded IN PLACE and gives
    its own results; another n_states, another prompt width (ld) and a prompt where none was give theirs; plain greedy, sampled and beam
    queue calls in between return what they returned before any constrained call."""
    eng, inp, shape, _, g = _case(be_name)
    eng.set_cross_absorb(False)
    try:
        order = ORDER[:7]
        q = _args(inp, order)
        V, eos, start = shape.vocab_size, shape.eos_token_id, shape.decoder_start_token_id
        geo = dict(max_length=T, chunk=4, slots=3, pool_chunks=2)
        bgeo = dict(geo, num_beams=3)

        def plain():
            a, b = eng.generate_stream(*q, **geo), eng.generate_stream_sampled(*q, **SKW, **geo)
            if be_name == "emu":      # (an emulated beam queue call takes tens of seconds, and nothing is captured there)
                return [_np(eng, x) for x in (a[0], a[1], b[0], b[1])]
            c = eng.generate_stream_beam(*q, **bgeo)
            return [_np(eng, x) for x in (a[0], a[1], b[0], b[1], c[0], c[1], c[2])]

        def same(x, y):
            return all(np.array_equal(_bits(i) if i.dtype == np.float32 else i, _bits(j) if j.dtype == np.float32 else j) for i, j in zip(x, y))

        def run(call=None, **kw):
            r = (call or eng.generate_stream)(*q, return_scores=True, **kw, **geo)
            return _np(eng, r[0]), _np(eng, r[1]), _np(eng, r[3])

        p0 = plain()
        a, b = K.suppress(V, eos, SUPPRESSED[:2]), K.suppress(V, eos, SUPPRESSED[2:])      # same sizes: one device buffer, refilled in place
        ra = run(constraint=a)
        assert same(ra, run(constraint=a))
        if be_name == "hip":
            assert eng.decode_graph_active()
        rb = run(constraint=b)
        assert not same(ra, rb)
        if be_name == "hip":
            assert eng.decode_graph_active()
        for n, im in enumerate(order):
            row, sc = _one_greedy(eng, inp, im, shape, constraint=b)
            assert rb[1][n] == len(row) and np.array_equal(rb[0][n, :len(row)], row) and np.array_equal(_bits(rb[2][n, :len(row) - 1]), _bits(sc)), n
        if be_name == "hip":      # (the interleaved plain calls are checked once more at the end on both backends)
            assert same(p0, plain())
        assert same(ra, run(constraint=a))
        c = K.begin_suppress(V, eos, SUPPRESSED)                                           # three states: another table, another key
        rc = run(constraint=c)
        assert same(rc[:2], p0[:2]), "the golden answers hold none of these tokens at column 1"
        if be_name == "hip":
            assert same(rb, run(constraint=b))
        # prompts: width 2, width 3 (another ld), none
        p2 = np.full((7, 2), start, np.int64)
        p2[:, 1] = [g["greedy_ids"][im][1] for im in order]
        r2 = run(constraint=a, constraint_start=np.zeros(7, np.int32), decoder_prompt=p2)
        p3 = np.concatenate([p2, p2[:, 1:]], axis=1)
        # (another ld is another key only where the step is captured: the emulator, which launches eagerly, skips the repeat)
        r3 = run(constraint=a, decoder_prompt=p3, decoder_prompt_len=np.full(7, 2, np.int32)) if be_name == "hip" else r2
        assert same(r2, r3) and same(r2[:2], ra[:2]), "column 1 of the suppressed rows is the golden token"
        assert np.all(r2[2][:, 0] == 0.0) and np.array_equal(_bits(r2[2][:, 1:]), _bits(ra[2][:, 1:]))
        assert same(ra, run(constraint=a))
        rs = run(eng.generate_stream_sampled, constraint=a, **SKW)
        assert same(rs, run(eng.generate_stream_sampled, constraint=a, **SKW)) and not same(rs[:2], ra[:2])
        assert same(p0, plain())
    finally:
        eng.set_cross_absorb("auto")


@pytest.mark.parametrize("be_name", BACKENDS)
def test_validation_names_the_argument(be_name):
    eng, inp, shape, _, g = _case(be_name)
    order = ORDER[:7]
    q = _args(inp, order)
    N = len(order)
    V, eos, start = shape.vocab_size, shape.eos_token_id, shape.decoder_start_token_id
    geo = dict(max_length=8, chunk=4, slots=3, pool_chunks=2)
    free = K.unconstrained(V, eos)
    ok = np.full((N, 3), 5, np.int64)
    ok[:, 0] = start
    calls = (eng.generate_stream, eng.generate_stream_sampled, lambda *a, **k: eng.generate_stream_beam(*a, num_beams=3, **k))
    ref = _np(eng, eng.generate_stream(*q, **geo)[0])

    def lens(v, at=N - 1):
        out = np.full(N, 2, np.int32)
        out[at] = v
        return out

    for call in calls:
        for bad, word in ((0, "length of image 6"), (4, "length of image 6"), (8, "below max_length")):
            pr = ok if bad != 8 else np.full((N, 9), start, np.int64)
            with pytest.raises(MgError, match=word) as e:
                call(*q, decoder_prompt=pr, decoder_prompt_len=lens(bad), **geo)
            assert "error -2" in str(e.value)
        for bad in (-1, free.n_states):
            st = np.zeros(N, np.int32)
            st[3] = bad
            with pytest.raises(MgError, match="start state of image 3") as e:
                call(*q, constraint=free, constraint_start=st, **geo)
            assert "error -2" in str(e.value)
        with pytest.raises(ValueError, match="decoder_prompt must be"):
            call(*q, decoder_prompt=ok[:3], **geo)
        with pytest.raises(ValueError, match="decoder_prompt_len must hold"):
            call(*q, decoder_prompt=ok, decoder_prompt_len=[2, 2], **geo)
        with pytest.raises(ValueError, match="constraint_start must hold"):
            call(*q, constraint=free, constraint_start=[0], **geo)
        with pytest.raises(ValueError, match="constraint_start needs constraint"):
            call(*q, constraint_start=np.zeros(N, np.int32), **geo)
        with pytest.raises(ValueError, match="vocabulary"):
            call(*q, constraint=K.unconstrained(V + 1, eos), **geo)
        with pytest.raises(TypeError):
            call(*q, constraint=lambda b, ids: [1], **geo)
    # a prompt id outside the vocabulary: replaced by 0, the call completes and returns MG_E_INPUT
    bad = ok.copy()
    bad[2, 1] = V
    bad[5, 0] = -3
    for call in calls:
        with pytest.raises(MgError, match="outside") as e:
            call(*q, decoder_prompt=bad, decoder_prompt_len=np.full(N, 2, np.int32), **geo)
        assert "error -8" in str(e.value)
    r = None
    try:
        eng.generate_stream(*q, decoder_prompt=bad, decoder_prompt_len=np.full(N, 2, np.int32), **geo)
    except MgError as e:
        r = e.outputs
    ids = _np(eng, r[0])
    assert ids[2, 1] == 0 and ids[5, 0] == 0 and ids[0, :2].tolist() == [start, 5]
    # the decode-capture instrumentation stays refused for queue calls
    eng.debug_decode_capture(capture_steps=2, rows=3)
    try:
        with pytest.raises(MgError) as e:
            eng.generate_stream(*q, constraint=free, **geo)
        assert "error -5" in str(e.value) or "instrumentation" in str(e.value)
    finally:
        eng.debug_decode_capture()
    assert np.array_equal(_np(eng, eng.generate_stream(*q, **geo)[0]), ref)
