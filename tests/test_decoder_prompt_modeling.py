"""model.generate(decoder_input_ids=, decoder_attention_mask=, max_new_tokens=, min_new_tokens=) on the trained tiny fixture: the keywords
are honoured as stock honours them (markushgrapher_amd/modeling.py _decoder_prompt), in every decode mode, and refused where the
feature is not built.  On the emulator the model's engine is replaced by one over the CPU backend (arrays come back as numpy); the
tuple outputs need torch tensors and run on the GPU only."""
import numpy as np
import pytest
import torch

from tests.backends import make_engine
from tests.conftest import load_golden
from tests.test_modeling import tiny_model
from tests.test_oracle_golden import _weights

BACKENDS = [pytest.param("emu"), pytest.param("hip", marks=pytest.mark.gpu)]
T = 16


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


@pytest.fixture
def case(request, monkeypatch):
    be_name = request.param
    m, shape = tiny_model()
    g = load_golden("g3_trained_tiny.npz")
    dev = "cpu"
    if be_name == "hip":
        m = m.to("cuda")
        dev = m.device
    else:
        eng = make_engine("emu", *_weights(g))
        monkeypatch.setattr(m, "_eng", lambda: eng)
    kw = {k: torch.from_numpy(g[k]).to(dev) for k in ("input_ids", "bbox", "attention_mask", "pixel_values")}
    return m, shape, kw, be_name


def _own_len(row, eos):
    e = np.flatnonzero(row[1:] == eos)
    return int(e[0]) + 1 if len(e) else len(row) - 1


def _padded(a, cols, pad):
    out = np.full((a.shape[0], cols), pad, a.dtype)
    out[:, :a.shape[1]] = a
    return out


@pytest.mark.parametrize("case", BACKENDS, indirect=True)
def test_generate_continues_its_own_prefix(case):
    """Before this feature the prompt was dropped: the last assertion of this test (a foreign prefix is kept) failed, the call returned y."""
    m, shape, kw, _ = case
    y = _np(m.generate(**kw, max_length=T))
    assert (y[:, 0] == shape.decoder_start_token_id).all()
    c = min(_own_len(r, shape.eos_token_id) for r in y)
    assert c >= 2
    for cut in sorted({2, c}):
        assert np.array_equal(_np(m.generate(**kw, max_length=T, decoder_input_ids=torch.from_numpy(y[:, :cut]))), y)
    # the start-token rule: no row starts with decoder_start_token_id -> it is prepended
    assert (y[:, 1] != shape.decoder_start_token_id).all()
    assert np.array_equal(_np(m.generate(**kw, max_length=T, decoder_input_ids=torch.from_numpy(y[:, 1:c]))), y)
    # sampled with the same seed (and the default stream ids): the same identity
    s = _np(m.generate(**kw, max_length=T, do_sample=True, seed=11, temperature=1.2))
    cs = min(_own_len(r, shape.eos_token_id) for r in s)
    assert np.array_equal(_np(m.generate(**kw, max_length=T, do_sample=True, seed=11, temperature=1.2,
                                         decoder_input_ids=torch.from_numpy(s[:, :cs]))), s)
    # a prefix the model would not write is kept, in every mode, and the answer goes on from it
    foreign = y[:, :3].copy()
    foreign[:, 2] = np.where(y[:, 2] == 7, 9, 7)
    for mode in (dict(), dict(num_beams=3), dict(do_sample=True, seed=5)):
        out = _np(m.generate(**kw, max_length=T, decoder_input_ids=torch.from_numpy(foreign), **mode))
        assert np.array_equal(out[:, :3], foreign) and out.shape[1] > 3, mode


@pytest.mark.parametrize("case", BACKENDS, indirect=True)
def test_some_row_with_the_start_token_means_no_prepend(case):
    m, shape, kw, _ = case
    B = kw["input_ids"].shape[0]
    dec = np.full((B, 3), 9, np.int64)
    dec[0, 0] = shape.decoder_start_token_id                      # stock prepends only if NO row starts with the start token
    out = _np(m.generate(**kw, max_length=8, decoder_input_ids=torch.from_numpy(dec)))
    assert np.array_equal(out[:, :3], dec)
    dec[0, 0] = 9
    out = _np(m.generate(**kw, max_length=8, decoder_input_ids=torch.from_numpy(dec)))
    assert (out[:, 0] == shape.decoder_start_token_id).all() and np.array_equal(out[:, 1:4], dec)


@pytest.mark.parametrize("case", BACKENDS, indirect=True)
def test_new_token_limits(case):
    m, shape, kw, _ = case
    eos, pad = shape.eos_token_id, shape.pad_token_id
    y = _np(m.generate(**kw, max_length=T))
    # without a prompt P = 1
    a = _np(m.generate(**kw, max_new_tokens=4))
    assert a.shape[1] <= 5 and np.array_equal(a, _np(m.generate(**kw, max_length=5)))
    p = torch.from_numpy(y[:, :3])
    b = _np(m.generate(**kw, max_new_tokens=4, decoder_input_ids=p))
    assert b.shape[1] <= 7 and np.array_equal(b, _np(m.generate(**kw, max_length=7, decoder_input_ids=p)))
    # min_new_tokens counts from the prompt's end and takes precedence over min_length
    n = 3 + 6
    c = _np(m.generate(**kw, max_length=T, min_new_tokens=6, min_length=2, decoder_input_ids=p))
    assert not (c[:, 3:n] == eos).any() and c.shape[1] >= n
    assert np.array_equal(c, _np(m.generate(**kw, max_length=T, min_length=n, decoder_input_ids=p)))
    d = _np(m.generate(**kw, max_length=T, min_new_tokens=6))
    assert np.array_equal(d, _np(m.generate(**kw, max_length=T, min_length=7)))
    own = np.array([_own_len(r, eos) for r in y])
    assert (own < n - 1).any(), "the fixture has rows that would stop earlier: min_new_tokens changed something"


@pytest.mark.parametrize("case", BACKENDS, indirect=True)
def test_lengths_come_from_the_mask(case):
    m, shape, kw, _ = case
    B = kw["input_ids"].shape[0]
    y = _np(m.generate(**kw, max_length=T))
    lens = np.array([1 + b % 4 for b in range(B)])
    dec = y[:, :4].copy()
    for b in range(B):
        dec[b, lens[b] - 1] = 9 if lens[b] > 1 else dec[b, 0]     # a foreign last token ...
        dec[b, lens[b]:] = shape.pad_token_id                     # ... and padding with the pad id, which is also the start id
    mask = (np.arange(4)[None, :] < lens[:, None]).astype(np.int64)
    out = _np(m.generate(**kw, max_length=T, decoder_input_ids=torch.from_numpy(dec), decoder_attention_mask=torch.from_numpy(mask)))
    for b in range(B):
        assert np.array_equal(out[b, :lens[b]], dec[b, :lens[b]])
        one = {k: v[b:b + 1] for k, v in kw.items()}
        alone = _np(m.generate(**one, max_length=T, decoder_input_ids=torch.from_numpy(dec[b:b + 1, :lens[b]])))
        assert np.array_equal(_padded(alone, out.shape[1], shape.pad_token_id), out[b:b + 1]), b
    # equal lengths below the width: the common length is the prompt
    mask2 = np.zeros((B, 4), np.int64)
    mask2[:, :2] = 1
    out2 = _np(m.generate(**kw, max_length=T, max_new_tokens=3, decoder_input_ids=torch.from_numpy(dec), decoder_attention_mask=torch.from_numpy(mask2)))
    ref2 = _np(m.generate(**kw, max_length=5, decoder_input_ids=torch.from_numpy(dec[:, :2])))
    assert np.array_equal(out2, ref2)
    # the mask gets its column of ones with the prepended start token
    nostart = np.full((B, 3), 9, np.int64)
    out3 = _np(m.generate(**kw, max_length=T, decoder_input_ids=torch.from_numpy(nostart), decoder_attention_mask=torch.from_numpy(mask[:, :3])))
    for b in range(B):
        n = min(lens[b], 3)
        assert out3[b, 0] == shape.decoder_start_token_id and (out3[b, 1:1 + n] == 9).all()


@pytest.mark.parametrize("case", BACKENDS, indirect=True)
def test_refusals(case):
    m, shape, kw, _ = case
    B = kw["input_ids"].shape[0]
    dec = torch.full((B, 4), 9, dtype=torch.long)
    dec[:, 0] = shape.decoder_start_token_id
    ragged = torch.ones((B, 4), dtype=torch.long)
    ragged[0, 2:] = 0

    def bad(**extra):
        with pytest.raises(ValueError):
            m.generate(**kw, **extra)
    hole = torch.ones((B, 4), dtype=torch.long)
    hole[1, 1] = 0
    left = torch.ones((B, 4), dtype=torch.long)
    left[1, 0] = 0
    empty = torch.ones((B, 4), dtype=torch.long)
    empty[1, :] = 0
    for mask in (hole, left, empty, torch.ones((B, 3), dtype=torch.long)):
        bad(max_length=T, decoder_input_ids=dec, decoder_attention_mask=mask)
    bad(max_length=T, decoder_attention_mask=ragged)                                     # a mask without ids
    bad(max_length=T, decoder_input_ids=dec[:1])                                         # another batch size
    bad(max_length=4, decoder_input_ids=dec)                                             # P >= max_length, as stock refuses it
    bad(max_length=3, decoder_input_ids=dec, decoder_attention_mask=ragged)              # ... for the longest row
    bad(max_length=T, max_new_tokens=3, decoder_input_ids=dec, decoder_attention_mask=ragged)      # per-row limits are not built
    bad(max_length=T, min_new_tokens=3, decoder_input_ids=dec, decoder_attention_mask=ragged)
    for mode in (dict(), dict(do_sample=True, seed=1)):
        bad(max_length=T, decoder_input_ids=dec, decoder_attention_mask=ragged, return_dict_in_generate=True, output_scores=True, **mode)
        bad(max_length=T, decoder_input_ids=dec, decoder_attention_mask=ragged, return_dict_in_generate=True, output_logits=True, **mode)
    # ragged prompts themselves are fine
    out = _np(m.generate(**kw, max_length=T, decoder_input_ids=dec, decoder_attention_mask=ragged))
    assert (out[1:, 1:4] == 9).all() and out[0, 1] == 9
    # the queue forms take no prompt: refused, where it used to be ignored
    enc = [{"input_ids": kw["input_ids"][b], "bbox": kw["bbox"][b], "pixel_values": kw["pixel_values"][b], "decoder_input_ids": dec[b:b + 1]}
           for b in range(2)]
    with pytest.raises(ValueError, match="decoder_input_ids"):
        m.generate_queue(enc, max_length=T)


@pytest.mark.gpu
def test_generate_output_holds_the_free_steps_only():
    """return_dict_in_generate with a prompt: sequences include it, token_scores are 0.0 in its columns, the scores / logits tuples hold one
    entry per FREE step, as stock's do (stock runs the prompt in one forward pass)."""
    m, shape = tiny_model()
    m = m.to("cuda")
    g = load_golden("g3_trained_tiny.npz")
    kw = {k: torch.from_numpy(g[k]).to(m.device) for k in ("input_ids", "bbox", "attention_mask", "pixel_values")}
    y = m.generate(**kw, max_length=T)
    P = 3
    p = y[:, :P].clone()
    p[:, P - 1] = torch.where(p[:, P - 1] == 7, 9, 7)
    for mode in (dict(), dict(num_beams=3, num_return_sequences=2), dict(do_sample=True, seed=2, top_k=0)):
        out = m.generate(**kw, max_length=T, decoder_input_ids=p, return_dict_in_generate=True, output_scores=True, output_logits=True, **mode)
        nr = mode.get("num_return_sequences", 1)
        seq = out.sequences
        assert torch.equal(seq[:, :P], p.repeat_interleave(nr, 0))
        assert len(out.scores) == len(out.logits) == seq.shape[1] - P
        assert torch.all(out.token_scores[:, :P - 1] == 0) and torch.all(out.token_scores[:, P - 1] < 0)
        if not mode:
            assert torch.equal(out.scores[0].argmax(-1), seq[:, P])
            ts = m.compute_transition_scores(seq, out.scores, normalize_logits=True)
            assert ts.shape[1] == seq.shape[1] - P
            live = torch.cumsum((seq[:, P:-1] == shape.eos_token_id).long(), 1) == 0
            live = torch.cat([torch.ones_like(live[:, :1]), live], 1)
            torch.testing.assert_close(ts[live], out.token_scores[:, P - 1:][live], atol=1e-3, rtol=0)
        if "num_beams" in mode:
            assert torch.all(out.beam_indices[:, :P - 1] >= 0)
