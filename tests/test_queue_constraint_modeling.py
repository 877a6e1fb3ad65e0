"""generate_queue_constrained(): the queue with the constraint options and per-encoding decoder prompts, against generate() on every
encoding alone with the same
options (the trained-tiny fixture; emu = the CPU SIMT emulator behind the model, hip = MI355X).  The queue is the fixture's 6 images and
image 0 again, on 3 slots with chunks of 2: every slot is handed over.

  each option alone      constraint / suppress_tokens / begin_suppress_tokens / bad_words_ids, three modes
  ragged prompts         decoder_input_ids 1-D, [1, P], absent, without the start token; with constraint_starts from constraint.one_of_each
  contexts               contexts=2 == contexts=1 (GPU: the emulator runs one context)
  refusals               what is refused names itself; generate_queue() itself keeps refusing prompt and options
"""
import numpy as np
import pytest
import torch

from markushgrapher_amd import constraint as K
from tests.test_decoder_prompt_modeling import BACKENDS, _np, case      # noqa: F401  (case: the fixture)
from tests.test_queue_constraint_engine import SUPPRESSED

T = 16
QUEUE = [0, 1, 2, 3, 4, 5, 0]
GEO = dict(max_length=T, slots=3, chunk=2)


def _one(kw, b):
    """image b as the reference's loop holds it: a batch of one, cut to its own text length (no padding)"""
    n = int(kw["attention_mask"][b].sum())
    return {"input_ids": kw["input_ids"][b:b + 1, :n], "bbox": kw["bbox"][b:b + 1, :n], "pixel_values": kw["pixel_values"][b:b + 1]}


def _encodings(kw, prompts=None, queue=None):
    enc = []
    for n, b in enumerate(QUEUE if queue is None else queue):
        e = _one(kw, b)
        if prompts is not None and prompts[n] is not None:
            e["decoder_input_ids"] = prompts[n]
        enc.append(e)
    return enc


def _alone(m, kw, b, **opts):
    return m.generate(**_one(kw, b), max_length=T, **opts)


def _cut(row, eos, first=1):
    row = _np(row)
    e = np.flatnonzero(row[first:] == eos)
    return row[:int(e[0]) + first + 1] if len(e) else row


def _modes(be_name):
    """greedy, sampled, beam-3 (beam-5 on the GPU: an emulated beam call takes seconds per row)"""
    return (dict(), dict(do_sample=True, seed=7, temperature=1.5, top_k=0), dict(num_beams=3 if be_name == "emu" else 5))


def _check(m, kw, eos, be_name, enc, per_entry, modes=None, **opts):
    """predictions[n] == generate(**encodings[n], the same options)[0] (cut at its EOS), in every mode"""
    for mode in (modes or _modes(be_name)):
        got = m.generate_queue_constrained(enc, **GEO, **mode, **opts)
        assert len(got) == len(QUEUE)
        for n, b in enumerate(QUEUE):
            extra = dict(per_entry[n]) if per_entry else {}
            first = int(torch.as_tensor(extra["decoder_input_ids"]).reshape(-1).shape[0]) if "decoder_input_ids" in extra else 1
            ref_mode = dict(mode, stream_ids=[n]) if mode.get("do_sample") else mode
            ref = _alone(m, kw, b, **dict(ref_mode, **dict(opts, **extra)))[0]
            want = _cut(ref, eos, max(1, first))
            assert np.array_equal(_np(got[n]), want), (mode, n, _np(got[n]).tolist(), want.tolist())
    return got


@pytest.mark.parametrize("case", BACKENDS, indirect=True)
@pytest.mark.parametrize("option", ["constraint", "suppress_tokens", "begin_suppress_tokens", "bad_words_ids"])
def test_each_option_equals_the_per_image_calls(case, option):
    """Non-vacuity: under suppress_tokens / constraint every greedy row leaves its golden answer at column 2; under begin_suppress_tokens
    at column 1; bad_words_ids bans the golden bigram of columns 1 - 2."""
    m, shape, kw, be_name = case
    V, eos = shape.vocab_size, shape.eos_token_id
    golden = [_np(r) for r in m.generate_queue_constrained(_encodings(kw), **GEO)[:6]]      # the plain queue's rows of the six images
    opts = {"constraint": dict(constraint=K.suppress(V, eos, SUPPRESSED)),
            "suppress_tokens": dict(suppress_tokens=list(SUPPRESSED)),
            "begin_suppress_tokens": dict(begin_suppress_tokens=sorted(set(int(r[1]) for r in golden))),
            "bad_words_ids": dict(bad_words_ids=[[int(r[1]), int(r[2])] for r in golden])}[option]
    got = _check(m, kw, eos, be_name, _encodings(kw), None, modes=_modes(be_name)[:1] if be_name == "emu" and option != "suppress_tokens" else None,
                 **opts)
    greedy = m.generate_queue_constrained(_encodings(kw), **GEO, **opts)
    col = 1 if option == "begin_suppress_tokens" else 2
    assert all(_np(greedy[n])[col] != golden[b][col] for n, b in enumerate(QUEUE))
    assert len(set(len(r) for r in greedy)) > 1


@pytest.mark.parametrize("case", BACKENDS, indirect=True)
def test_ragged_prompts_and_one_of_each(case):
    """Entry n answers with the golden answer of image (b + 2) % 6 or (b + 3) % 6 (constraint.one_of_each: a root per entry, passed as
    constraint_starts); entries 1, 4 carry a 1-D prompt [start, first token of their first candidate], entry 2 a [1, 2] prompt WITHOUT
    the start token (prepended, as generate() does for a batch of one), the others none.  Every prediction is a candidate of its entry
    followed by EOS and equals generate() on that encoding with constraint_starts=[root]."""
    m, shape, kw, be_name = case
    V, eos, start = shape.vocab_size, shape.eos_token_id, shape.decoder_start_token_id
    golden = [_np(r) for r in m.generate_queue_constrained(_encodings(kw), **GEO)[:6]]
    ans = [[int(t) for t in r[1:-1]] for r in golden]
    cands = [[ans[(b + 2) % 6], ans[(b + 3) % 6]] for b in QUEUE]
    aut, roots = K.one_of_each(V, eos, cands)
    prompts = [None] * len(QUEUE)
    prompts[1] = torch.tensor([start, cands[1][0][0]])
    prompts[4] = torch.tensor([start, cands[4][0][0]])
    prompts[2] = torch.tensor([[cands[2][1][0], cands[2][1][1]]])
    per_entry = [dict(constraint_starts=[int(roots[n])], **({} if prompts[n] is None else dict(decoder_input_ids=prompts[n].reshape(1, -1))))
                 for n in range(len(QUEUE))]
    for n in (2,):      # generate() prepends the start token too: the reference's prompt is one column longer than what was passed
        per_entry[n]["decoder_input_ids"] = torch.cat([torch.tensor([[start]]), prompts[n]], dim=-1)
    got = _check(m, kw, eos, be_name, _encodings(kw, prompts), per_entry, constraint=aut, constraint_starts=roots)
    for n in range(len(QUEUE)):
        row = [int(t) for t in _np(got[n])]
        assert row[0] == start and row[-1] == eos and row[1:-1] in cands[n], (n, row, cands[n])
    assert [int(t) for t in _np(got[2])[1:3]] == cands[2][1][:2]


@pytest.mark.gpu
def test_contexts_2_equals_contexts_1():
    """the queue cut over two execution contexts: each part gets its slice of prompts and start states"""
    from tests.conftest import load_golden
    from tests.test_modeling import tiny_model
    m, shape = tiny_model()
    m = m.to("cuda")
    g = load_golden("g3_trained_tiny.npz")
    kw = {k: torch.from_numpy(g[k]).to(m.device) for k in ("input_ids", "bbox", "attention_mask", "pixel_values")}
    V, eos, start = shape.vocab_size, shape.eos_token_id, shape.decoder_start_token_id
    golden = _np(m.generate(**kw, max_length=T))
    ans = [[int(t) for t in _cut(r, eos)[1:-1]] for r in golden]
    order = QUEUE + QUEUE
    cands = [[ans[(b + 2) % 6], ans[(b + 3) % 6]] for b in order]
    aut, roots = K.one_of_each(V, eos, cands)
    enc = _encodings(kw, [torch.tensor([start, cands[n][0][0]]) if n % 3 == 1 else None for n in range(len(order))], order)
    for mode in (dict(), dict(do_sample=True, seed=7, temperature=1.5, top_k=0), dict(num_beams=5)):
        one = m.generate_queue_constrained(enc, max_length=T, slots=3, chunk=2, constraint=aut, constraint_starts=roots, suppress_tokens=[9], **mode)
        two = m.generate_queue_constrained(enc, max_length=T, slots=3, chunk=2, contexts=2, constraint=aut, constraint_starts=roots, suppress_tokens=[9], **mode)
        assert len(one) == len(two) == len(order)
        for n in range(len(order)):
            assert np.array_equal(_np(one[n]), _np(two[n])), (mode, n)
            assert [int(t) for t in _np(one[n])[1:-1]] in cands[n], (mode, n)


@pytest.mark.parametrize("case", BACKENDS, indirect=True)
def test_refusals_and_what_is_no_longer_refused(case):
    m, shape, kw, be_name = case
    V, eos, start = shape.vocab_size, shape.eos_token_id, shape.decoder_start_token_id
    enc = _encodings(kw)[:3]
    for k, v in (("max_new_tokens", 4), ("min_new_tokens", 2), ("output_scores", True), ("prefix_allowed_tokens_fn", len),
                 ("repetition_penalty", 1.2), ("no_repeat_ngram_size", 2)):
        with pytest.raises(ValueError, match=k):
            m.generate_queue_constrained(enc, max_length=T, **{k: v})
    with pytest.raises(TypeError):
        m.generate_queue_constrained(enc, max_length=T, no_such_keyword=1)
    with pytest.raises(ValueError, match="constraint_starts"):
        m.generate_queue_constrained(enc, max_length=T, constraint_starts=[0, 0, 0])
    free = K.unconstrained(V, eos)
    with pytest.raises(ValueError, match="constraint_starts"):
        m.generate_queue_constrained(enc, max_length=T, constraint=free, constraint_starts=[0, 0])
    with pytest.raises(ValueError, match="constraint_starts"):
        m.generate_queue_constrained(enc, max_length=T, constraint=free, constraint_starts=[0, 0, free.n_states])
    with pytest.raises(ValueError, match="constraint_starts"):
        m.generate(**{k: kw[k][:2] for k in ("input_ids", "bbox", "pixel_values", "attention_mask")}, max_length=T, constraint=free, constraint_starts=[0])
    bad = [dict(e) for e in enc]
    bad[1]["decoder_input_ids"] = torch.zeros((2, 3), dtype=torch.long)
    with pytest.raises(ValueError, match="decoder_input_ids"):
        m.generate_queue_constrained(bad, max_length=T)
    bad[1]["decoder_input_ids"] = torch.full((T,), 9, dtype=torch.long)
    with pytest.raises(ValueError, match="decoder prompt"):
        m.generate_queue_constrained(bad, max_length=T)
    bad[1] = dict(enc[1], decoder_attention_mask=torch.ones((1, 2), dtype=torch.long))
    with pytest.raises(ValueError, match="decoder_attention_mask"):
        m.generate_queue_constrained(bad, max_length=T)
    # the neutral values pass; the unconstrained automaton and a [start] prompt give the plain queue's predictions - generate_queue()'s,
    # which keeps refusing both by name
    plain = m.generate_queue(enc, **GEO)
    with pytest.raises(ValueError, match="constraint"):
        m.generate_queue(enc, **GEO, constraint=K.unconstrained(V, eos))
    with pytest.raises(ValueError, match="decoder_input_ids"):
        m.generate_queue([dict(e, decoder_input_ids=torch.tensor([start])) for e in enc], **GEO)
    withp = [dict(e, decoder_input_ids=torch.tensor([start])) for e in enc]
    for got in (m.generate_queue_constrained(enc, **GEO, repetition_penalty=1.0, no_repeat_ngram_size=0), m.generate_queue_constrained(enc, **GEO, constraint=free),
                m.generate_queue_constrained(withp, **GEO), m.generate_queue_constrained(enc, **GEO, suppress_tokens=[], bad_words_ids=None)):
        assert all(np.array_equal(_np(a), _np(b)) for a, b in zip(got, plain))
