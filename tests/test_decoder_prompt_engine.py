"""The decoder prompt at engine level: mg_generate_prompted through Engine.generate(decoder_prompt=) / generate_sampled(decoder_prompt=)
(include/mgrapher.h mg_decoder_prompt) on the tiny fixtures.

  self-prefix identity   a prompt cut from what the same call emits unprompted gives the same ids, length and free-column token scores, bit
                         for bit: greedy (fused and unfused tail) and sampled, ragged cuts, eager / captured graph / device-counter form;
                         a [start] prompt in beam mode is the unprompted beam call
  foreign prompt         the continuation of a prefix the model would not have written, against the fp32 oracle's teacher-forced logits
  beam                   stock's identity sum(token scores) / generated length ^ penalty = sequence score with the prompt excluded, and
                         the token scores against the oracle
  per-image semantics    row b of a ragged batch = the call on image b alone with its prompt (cross-attention form pinned)
  validation             every error the header lists
"""
import ctypes as C

import numpy as np
import pytest
import torch

from markushgrapher_amd.engine import MgDecoderPrompt, MgError, MgSampleOpts
from oracle.udop_oracle import Oracle
from tests.backends import make_engine
from tests.conftest import load_golden
from tests.test_oracle_golden import _inputs, _weights
from tests.test_sampling_engine import _absorb_settings, _np, _same_ids
from tests.test_scores import TOL, _log_softmax

BACKENDS = [pytest.param("emu"), pytest.param("hip", marks=pytest.mark.gpu)]
FIXTURES = ["g3_trained_tiny.npz", "g0_tiny.npz"]
NEVER_READ = 10 ** 6         # columns of the prompt buffer past a row's length


def _case(be_name, fixture, T=None):
    g = load_golden(fixture)
    shape, sd = _weights(g)
    inp = _inputs(g, shape)
    eng = make_engine(be_name, shape, sd)
    full = int(g["max_length"]) if "max_length" in g else 16
    return eng, (inp["input_ids"], inp["bbox"], inp["attention_mask"], inp["pixel_values"]), shape, sd, min(T or full, 24)


def _modes(be_name):
    return (0, 2) if be_name == "emu" else (1, 0, 2)


def _own_len(row, eos):
    """columns a row wrote itself before its EOS (the start token included): a prompt up to there is a proper prefix"""
    e = np.flatnonzero(row[1:] == eos)
    return int(e[0]) + 1 if len(e) else len(row) - 1


def _cuts(ids, eos):
    """three cuts per row, ragged across the batch: the start token alone, the middle, everything the row wrote before its EOS"""
    n = np.array([max(1, _own_len(r, eos)) for r in ids])
    mid = np.maximum(1, (n + np.arange(len(n)) % 2) // 2)
    return [np.ones(len(n), np.int32), mid.astype(np.int32), n.astype(np.int32)]


def _prompt(ids, lens):
    P = int(max(lens))
    p = np.full((ids.shape[0], P), NEVER_READ, np.int64)
    for b, n in enumerate(lens):
        p[b, :n] = ids[b, :n]
    return p


def _check_identity(base_ids, base_ts, ids, ts, lens):
    assert ids.shape == base_ids.shape and np.array_equal(ids, base_ids)
    for b, n in enumerate(lens):
        assert np.all(ts[b, :n - 1] == 0)                                                        # forced columns score 0
        assert np.array_equal(ts[b, n - 1:].view(np.uint32), base_ts[b, n - 1:].view(np.uint32))  # free columns: the same bits


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("fixture", FIXTURES)
@pytest.mark.parametrize("fused", ["1", "0"], ids=["fused", "unfused"])
def test_self_prefix_identity_greedy(be_name, fixture, fused, monkeypatch):
    monkeypatch.setenv("MG_DECODE_FUSED_TAIL", fused)            # read when the engine is created
    eng, args, shape, _, T = _case(be_name, fixture)
    for mode in _modes(be_name):
        eng.set_decode_graph(mode)
        try:
            ids0, _, _, ex = eng.generate(*args, max_length=T, return_scores=True)
            ids0, ts0 = _np(eng, ids0), _np(eng, ex["token_scores"])
            for lens in _cuts(ids0, shape.eos_token_id):
                for _ in range(2):                               # the second call of a shape replays the captured step
                    ids, _, _, ex = eng.generate(*args, max_length=T, return_scores=True, decoder_prompt=_prompt(ids0, lens),
                                                 decoder_prompt_len=lens)
                    _check_identity(ids0, ts0, _np(eng, ids), _np(eng, ex["token_scores"]), lens)
                    if mode == 1:
                        assert eng.decode_graph_active()
            plain, _, _ = eng.generate(*args, max_length=T, decoder_prompt=_prompt(ids0, lens), decoder_prompt_len=lens)      # unscored entry
            assert np.array_equal(_np(eng, plain), ids0)
        finally:
            eng.set_decode_graph(1)


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("fixture", FIXTURES)
def test_self_prefix_identity_sampled(be_name, fixture):
    eng, args, shape, _, T = _case(be_name, fixture, T=16)
    B = args[0].shape[0]
    for nr in (1, 2):
        kw = dict(max_length=T, temperature=1.3, top_k=20, top_p=0.95, seed=41, num_return=nr, stream_ids=np.arange(B * nr) * 5 + 2,
                  return_scores=True)
        for mode in _modes(be_name):
            eng.set_decode_graph(mode)
            try:
                ids0, _, ts0 = eng.generate_sampled(*args, **kw)
                ids0, ts0 = _np(eng, ids0), _np(eng, ts0)
                # image b's samples share its prompt: cut from sample 0, so the other samples of the image follow a foreign prefix - only
                # sample 0 of every image is compared with the unprompted call (with num_return = 1 that is every row)
                for lens in _cuts(ids0[::nr], shape.eos_token_id):
                    ids, _, ts = eng.generate_sampled(*args, decoder_prompt=_prompt(ids0[::nr], lens), decoder_prompt_len=lens, **kw)
                    ids, ts = _np(eng, ids), _np(eng, ts)
                    for j in range(nr):
                        for b, n in enumerate(lens):
                            assert np.array_equal(ids[b * nr + j, :n], ids0[b * nr, :n]) and np.all(ts[b * nr + j, :n - 1] == 0)
                    m = min(ids.shape[1], ids0.shape[1])
                    assert _same_ids(ids[::nr], ids0[::nr], shape.pad_token_id)
                    for b, n in enumerate(lens):
                        assert np.array_equal(ts[b * nr, n - 1:m - 1].view(np.uint32), ts0[b * nr, n - 1:m - 1].view(np.uint32))
                    if mode == 1:
                        assert eng.decode_graph_active()
            finally:
                eng.set_decode_graph(1)


@pytest.mark.parametrize("be_name", BACKENDS)
def test_start_prompt_is_the_unprompted_call_in_every_mode(be_name):
    eng, args, shape, _, T = _case(be_name, "g3_trained_tiny.npz", T=12)
    B = args[0].shape[0]
    start = np.full((B, 1), shape.decoder_start_token_id, np.int64)
    for mode in _modes(be_name):
        eng.set_decode_graph(mode)
        try:
            a = eng.generate(*args, num_beams=3, max_length=T, num_return=3, return_scores=True, length_penalty=0.7)
            b = eng.generate(*args, num_beams=3, max_length=T, num_return=3, return_scores=True, length_penalty=0.7, decoder_prompt=start)
            for x, y in ((a[0], b[0]), (a[1], b[1]), (a[3]["token_scores"], b[3]["token_scores"]), (a[3]["beam_indices"], b[3]["beam_indices"])):
                x, y = _np(eng, x), _np(eng, y)
                assert x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), mode
            g = eng.generate(*args, max_length=T, return_scores=True)
            p = eng.generate(*args, max_length=T, return_scores=True, decoder_prompt=start)
            assert np.array_equal(_np(eng, g[0]), _np(eng, p[0]))
            assert np.array_equal(_np(eng, g[3]["token_scores"]).view(np.uint32), _np(eng, p[3]["token_scores"]).view(np.uint32))
            kw = dict(max_length=T, temperature=1.2, seed=3, return_scores=True)
            s, q = eng.generate_sampled(*args, **kw), eng.generate_sampled(*args, decoder_prompt=start, **kw)
            assert np.array_equal(_np(eng, s[0]), _np(eng, q[0])) and np.array_equal(_np(eng, s[2]).view(np.uint32), _np(eng, q[2]).view(np.uint32))
        finally:
            eng.set_decode_graph(1)


def _foreign(ids, shape, cuts):
    """the greedy output up to column c_b, then a different valid token that stops nothing"""
    lens = np.array([c + 1 for c in cuts], np.int32)
    p = _prompt(ids, lens)
    for b, c in enumerate(cuts):
        t = (int(ids[b, c]) + 1) % shape.vocab_size
        while t in (shape.eos_token_id, shape.pad_token_id, int(ids[b, c])):
            t = (t + 1) % shape.vocab_size
        p[b, c] = t
    return p, lens


def _oracle_logprobs(shape, sd, args, ids):
    """teacher-forced log-softmax of the fp32 oracle: entry [b, j] scores the token in column j + 1 of ids"""
    with torch.no_grad():
        lg = Oracle(shape, sd).forward(args[0], args[1], args[3], args[2], decoder_input_ids=ids[:, :-1]).numpy().astype(np.float64)
    return lg, _log_softmax(lg)


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("fixture", FIXTURES)
def test_foreign_prompt_against_the_oracle(be_name, fixture):
    eng, args, shape, sd, T = _case(be_name, fixture)
    ids0, _, _ = eng.generate(*args, max_length=T)
    ids0 = _np(eng, ids0)
    cuts = [max(1, min(_own_len(r, shape.eos_token_id) - 1, 2 + b % 3)) for b, r in enumerate(ids0)]
    prompt, lens = _foreign(ids0, shape, cuts)
    ids, _, _, ex = eng.generate(*args, max_length=T, return_scores=True, decoder_prompt=prompt, decoder_prompt_len=lens)
    ids, ts = _np(eng, ids), _np(eng, ex["token_scores"])
    lg, lp = _oracle_logprobs(shape, sd, args, ids)
    worst_ts = worst_gap = 0.0
    for b, n in enumerate(lens):
        assert np.array_equal(ids[b, :n], prompt[b, :n]) and np.all(ts[b, :n - 1] == 0)
        e = np.flatnonzero(ids[b, n:] == shape.eos_token_id)      # the row's own EOS: searched from its first free column on
        last = int(n + e[0]) if len(e) else ids.shape[1] - 1
        for col in range(n, last + 1):                            # every free column the row wrote itself, none excluded
            tok = int(ids[b, col])
            worst_ts = max(worst_ts, abs(ts[b, col - 1] - lp[b, col - 1, tok]))
            worst_gap = max(worst_gap, lg[b, col - 1].max() - lg[b, col - 1, tok])
        assert np.all(ts[b, last:] == 0) and np.all(ids[b, last + 1:] == shape.pad_token_id)
    print(f"{fixture}: max |token score - oracle| = {worst_ts:.4f}, max oracle gap of an emitted token = {worst_gap:.4f} (bound {TOL})")
    # TOL is twice the logit tolerance of the tiny fixtures: the engine's choice has its own largest logit, each of the two logits is off
    # by at most the logit tolerance
    assert worst_ts < TOL and worst_gap <= TOL


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("length_penalty", [1.0, 0.7])
def test_beam_with_a_prompt(be_name, length_penalty):
    eng, args, shape, sd, T = _case(be_name, "g3_trained_tiny.npz", T=16)
    K = 5
    ids0, _, _ = eng.generate(*args, max_length=T)
    ids0 = _np(eng, ids0)
    cuts = [max(1, min(_own_len(r, shape.eos_token_id) - 1, 1 + b % 4)) for b, r in enumerate(ids0)]
    prompt, lens = _foreign(ids0, shape, cuts)
    ids, sc, _, ex = eng.generate(*args, num_beams=K, max_length=T, num_return=K, return_scores=True, length_penalty=length_penalty,
                                  decoder_prompt=prompt, decoder_prompt_len=lens)
    ids, sc, ts, bi = _np(eng, ids), _np(eng, sc), _np(eng, ex["token_scores"]), _np(eng, ex["beam_indices"])
    _, lp = _oracle_logprobs(shape, sd, tuple(np.repeat(a, K, 0) for a in args), ids)
    assert (sc > -1e8).all()
    for r in range(ids.shape[0]):
        b, n = r // K, int(lens[r // K])
        assert np.array_equal(ids[r, :n], prompt[b, :n])
        assert np.all(bi[r, :n - 1] == b * K) and np.all(ts[r, :n - 1] == 0)                     # forced columns: beam-0 flat row, score 0
        gen = int((bi[r] >= 0).sum()) - (n - 1)                                                  # generated tokens of the hypothesis
        assert gen >= 1 and np.all(bi[r, n - 1 + gen:] == -1)
        np.testing.assert_allclose(ts[r].astype(np.float64).sum() / float(gen) ** length_penalty, sc[r], rtol=1e-5, atol=1e-6)
        want = lp[r, np.arange(n - 1, n - 1 + gen), ids[r, n:n + gen]]
        np.testing.assert_allclose(ts[r, n - 1:n - 1 + gen], want, atol=TOL)
        assert np.all(np.diff(sc[b * K:(b + 1) * K]) <= 0)                                       # best first


@pytest.mark.parametrize("be_name", BACKENDS)
def test_ragged_batch_rows_equal_one_image_calls(be_name):
    """Property 2, compared as tests/test_sampling_engine.py::test_call_size_independence compares: ids, with the cross-attention form pinned."""
    eng, args, shape, _, T = _case(be_name, "g0_tiny.npz", T=10)
    B = args[0].shape[0]
    ids0, _, _ = eng.generate(*args, max_length=T, min_length=T)
    prompt, lens = _foreign(_np(eng, ids0), shape, [1 + b % 4 for b in range(B)])
    sid = np.arange(B) * 7 + 3
    skw = dict(max_length=T, min_length=T, temperature=1.3, top_k=20, top_p=0.95, seed=77)
    for absorb in _absorb_settings(eng):
        eng.set_cross_absorb(absorb)
        try:
            g, _, _ = eng.generate(*args, max_length=T, min_length=T, decoder_prompt=prompt, decoder_prompt_len=lens)
            bm, bsc, _ = eng.generate(*args, num_beams=3, max_length=T, decoder_prompt=prompt, decoder_prompt_len=lens)
            s, _, _ = eng.generate_sampled(*args, stream_ids=sid, decoder_prompt=prompt, decoder_prompt_len=lens, **skw)
            g, bm, s = _np(eng, g), _np(eng, bm), _np(eng, s)
            fill = shape.pad_token_id or shape.eos_token_id
            for b in range(B):
                one = tuple(a[b:b + 1] for a in args)
                pb, lb = prompt[b:b + 1, :lens[b]], lens[b:b + 1]
                g1, _, _ = eng.generate(*one, max_length=T, min_length=T, decoder_prompt=pb, decoder_prompt_len=lb)
                assert np.array_equal(_np(eng, g1), g[b:b + 1]), (absorb, "greedy", b)
                b1, _, _ = eng.generate(*one, num_beams=3, max_length=T, decoder_prompt=pb, decoder_prompt_len=lb)
                assert _same_ids(_np(eng, b1), bm[b:b + 1], fill), (absorb, "beam", b)      # (the batch returns its longest hypothesis' columns)
                s1, _, _ = eng.generate_sampled(*one, stream_ids=sid[b:b + 1], decoder_prompt=pb, decoder_prompt_len=lb, **skw)
                assert np.array_equal(_np(eng, s1), s[b:b + 1]), (absorb, "sampled", b)
        finally:
            eng.set_cross_absorb("auto")


def _code(excinfo):
    return int(str(excinfo.value).split("error ")[1].split(":")[0])


@pytest.mark.parametrize("be_name", BACKENDS)
def test_validation(be_name):
    eng, args, shape, _, T = _case(be_name, "g3_trained_tiny.npz", T=8)
    B = args[0].shape[0]
    ok = np.full((B, 3), 5, np.int64)
    ok[:, 0] = shape.decoder_start_token_id

    def lens(v):
        out = np.full(B, 2, np.int32)
        out[B - 1] = v
        return out
    for bad_len in (0, 4, -1):                                    # 1 <= len <= ld
        with pytest.raises(MgError) as e:
            eng.generate(*args, max_length=T, decoder_prompt=ok, decoder_prompt_len=lens(bad_len))
        assert _code(e) == -2 and "prompt" in str(e.value)
    wide = np.full((B, T), 5, np.int64)
    with pytest.raises(MgError) as e:                             # len < max_length
        eng.generate(*args, max_length=T, decoder_prompt=wide, decoder_prompt_len=lens(T))
    assert _code(e) == -2 and "max_length" in str(e.value)
    eng.generate(*args, max_length=T, decoder_prompt=wide, decoder_prompt_len=lens(T - 1))       # one free column is a call
    for mode in ("greedy", "beam", "sampled"):                    # the same checks in front of every mode
        with pytest.raises(MgError) as e:
            if mode == "sampled":
                eng.generate_sampled(*args, max_length=T, decoder_prompt=ok, decoder_prompt_len=lens(0))
            else:
                eng.generate(*args, num_beams=1 if mode == "greedy" else 3, max_length=T, decoder_prompt=ok, decoder_prompt_len=lens(0))
        assert _code(e) == -2
    with pytest.raises(ValueError):
        eng.generate(*args, max_length=T, decoder_prompt=ok[:1])
    with pytest.raises(ValueError):
        eng.generate(*args, max_length=T, decoder_prompt=ok, decoder_prompt_len=[1])
    with pytest.raises(ValueError):
        eng.generate(*args, max_length=T, decoder_prompt_len=lens(1))
    # a prompt id outside [0, vocab): MG_E_INPUT, as for encoder ids - in a forced column of each mode and in column 0
    for col in (0, 1):
        for mode in ("greedy", "beam", "sampled"):
            bad = ok.copy()
            bad[1, col] = shape.vocab_size + 3 if mode != "beam" else -1
            with pytest.raises(MgError) as e:
                if mode == "sampled":
                    eng.generate_sampled(*args, max_length=T, decoder_prompt=bad)
                else:
                    eng.generate(*args, num_beams=1 if mode == "greedy" else 3, max_length=T, decoder_prompt=bad)
            assert _code(e) == -8, (col, mode)
    bad = ok.copy()
    bad[1, 2] = shape.vocab_size + 3                              # ... but not past the row's length: never read
    eng.generate(*args, max_length=T, decoder_prompt=bad, decoder_prompt_len=np.full(B, 2, np.int32))
    # with mg_debug_decode_capture's forced ids: unsupported; its logits capture alone keeps working
    eng.debug_decode_capture(capture_steps=2, rows=B, forced_ids=np.zeros((B, T), np.int64))
    try:
        with pytest.raises(MgError) as e:
            eng.generate(*args, max_length=T, decoder_prompt=ok)
        assert _code(e) == -5
    finally:
        eng.debug_decode_capture()
    ref, _, _ = eng.generate(*args, max_length=T, decoder_prompt=ok)
    cap = eng.debug_decode_capture(capture_steps=T - 1, rows=B)
    try:
        ids, _, _ = eng.generate(*args, max_length=T, decoder_prompt=ok)
    finally:
        eng.debug_decode_capture()
    ids, cap = _np(eng, ids), _np(eng, cap)
    assert np.array_equal(ids, _np(eng, ref))
    assert np.array_equal(cap[2].argmax(-1)[: B], ids[:, 3])     # step 2 writes column 3, the first free one
    # the C entry itself: a sampled call takes num_beams = 1; a NULL prompt is the unprompted call (checked through Engine above)
    samp = MgSampleOpts(1.0, 0, 1.0, 1, None, 1, None)
    cols = C.c_int(0)
    rc = eng.lib.mg_generate_prompted(eng.model, None, None, 0, None, None, None, None, None, 0, B, 4, 2, T, 0, C.c_float(1.0), 0, None,
                                      C.byref(cols), None, None, None, C.byref(samp), None)
    assert rc == -2 and b"num_beams" in eng.lib.mg_last_error()
    p = MgDecoderPrompt(None, None, 3)
    rc = eng.lib.mg_generate_prompted(eng.model, None, None, 0, None, None, None, None, None, 0, B, 4, 1, T, 0, C.c_float(1.0), 0,
                                      C.c_void_p(8), C.byref(cols), None, None, None, None, C.byref(p))
    assert rc == -2 and b"prompt" in eng.lib.mg_last_error()
    need, base = C.c_size_t(), C.c_size_t()
    L = int(args[0].shape[1])
    assert eng.lib.mg_prompted_workspace_bytes(eng.model, B, L, 3, T, 0, 0, C.byref(need)) == 0
    assert eng.lib.mg_workspace_bytes(eng.model, B, L, 3, T, 0, 0, C.byref(base)) == 0
    assert base.value < need.value <= base.value + 256 * ((4 * B + 255) // 256)
