"""Scoring through the engine (include/mgrapher.h mg_decoder_score / mg_score_workspace_bytes; Engine.score / Engine.score_candidates) on the
tiny fixtures.

  logits path  token / argmax log-probabilities against the float64 log-softmax of Engine.forward_logits on the same inputs: both paths run
               the same decoder stack and the same k-ascending MFMA chains per logit, so what separates them is the fp32 exp / log of the
               fused epilogue against float64 - 1e-3 leaves two orders of magnitude; the argmax is compared wherever the logits' top-2 gap
               exceeds 1e-3, and on the trained fixture at most 2 % of the positions may fall under it
  unchanged    forward_logits gives the same bits before and after a score() call and in a fresh engine that scored first;
               mg_workspace_bytes returns the parent commit's numbers
  candidates   score_candidates = separate score calls, bit for bit; greedy generate()'s token scores = score() of the generated ids
               within tests/test_scores.py's TOL (two independent code paths: decode step and teacher-forced forward)
  errors       MG_E_INPUT / MG_E_SHAPE / MG_E_WORKSPACE / MG_E_STATE"""
import ctypes as C
import hashlib

import numpy as np
import pytest

from tests.backends import make_engine
from tests.conftest import load_golden
from tests.test_oracle_golden import _inputs, _weights

BACKENDS = [pytest.param("emu"), pytest.param("hip", marks=pytest.mark.gpu)]
TOL = 0.05          # tests/test_scores.py
GAP = 1e-3
MG_E_SHAPE, MG_E_STATE, MG_E_WORKSPACE, MG_E_INPUT = -1, -3, -6, -8

# mg_workspace_bytes(model, B, L, 1, 0, T, 0) of the tiny shape, recorded from the parent commit's emulator build: {(B, L, T): bytes}
PARENT_WS = {
    (1, 8, 0): 203520, (1, 8, 5): 347904, (1, 8, 64): 352000, (1, 8, 65): 463360,
    (1, 70, 0): 364032, (1, 70, 5): 541184, (1, 70, 64): 545280, (1, 70, 65): 656640,
    (3, 8, 0): 549120, (3, 8, 5): 973568, (3, 8, 64): 994048, (3, 8, 65): 1320192,
    (3, 70, 0): 1031168, (3, 70, 5): 1553920, (3, 70, 64): 1574400, (3, 70, 65): 1900544,
    (6, 8, 0): 1039360, (6, 8, 5): 1884160, (6, 8, 64): 1929216, (6, 8, 65): 2577152,
    (6, 70, 0): 2002944, (6, 70, 5): 3044352, (6, 70, 64): 3089408, (6, 70, 65): 3737344,
}


def _np(eng, h):
    return eng.mem.numpy(h)


def _case(be_name, fixture):
    g = load_golden(fixture)
    shape, sd = _weights(g)
    inp = _inputs(g, shape)
    eng = make_engine(be_name, shape, sd)
    args = (inp["input_ids"], inp["bbox"], inp["attention_mask"], inp["pixel_values"])
    labels = np.asarray(g["labels"]).astype(np.int64)
    dec = np.zeros_like(labels)
    dec[:, 1:] = labels[:, :-1]
    dec[:, 0] = shape.decoder_start_token_id
    dec[dec == -100] = shape.pad_token_id
    return g, shape, eng, args, labels, dec


def _log_softmax64(x):
    x = x.astype(np.float64)
    m = x.max(-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("fixture", ["g3_trained_tiny.npz", "g0_tiny.npz"])
def test_score_agrees_with_the_logits_path(be_name, fixture):
    g, shape, eng, args, labels, dec = _case(be_name, fixture)
    dam = (labels != -100).astype(np.uint8)
    logits = _np(eng, eng.forward_logits(*args, dec, dam)[0]).copy()
    tok, arg, alp = (_np(eng, a) for a in eng.score(*args, dec, labels, dam))
    lp = _log_softmax64(logits)
    live = labels >= 0
    ref_tok = np.where(live, np.take_along_axis(lp, np.where(live, labels, 0)[..., None], -1)[..., 0], 0.0)
    print("token_logprobs max abs error", np.abs(tok - ref_tok).max(), "argmax_logprobs", np.abs(alp - lp.max(-1)).max())
    assert np.abs(tok - ref_tok).max() < 1e-3
    assert np.all(tok[~live] == 0.0)
    assert np.abs(alp - lp.max(-1)).max() < 1e-3
    top2 = np.sort(logits.astype(np.float64), -1)[..., -2:]
    decided = (top2[..., 1] - top2[..., 0]) > GAP
    assert np.array_equal(arg[decided], logits.argmax(-1)[decided])
    assert np.all((arg >= 0) & (arg < shape.vocab_size))
    if fixture.startswith("g3"):                     # trained: wide margins.  (The untrained fixture's share is not asserted.)
        print("share of positions under the gap", 1.0 - decided.mean())
        assert 1.0 - decided.mean() <= 0.02


@pytest.mark.parametrize("be_name", BACKENDS)
def test_forward_logits_is_unchanged_by_scoring(be_name):
    g, shape, eng, args, labels, dec = _case(be_name, "g3_trained_tiny.npz")
    h = lambda e: hashlib.sha256(_np(e, e.forward_logits(*args, dec)[0]).tobytes()).hexdigest()
    before = h(eng)
    eng.score(*args, dec, labels)
    assert h(eng) == before                          # the same engine, after a score() call (its workspace grew in between)
    _, _, eng2, _, _, _ = _case(be_name, "g3_trained_tiny.npz")
    eng2.score(*args, dec, labels)
    assert h(eng2) == before                         # a fresh engine that scored first
    need = C.c_size_t()
    for (B, L, T), nbytes in PARENT_WS.items():
        assert eng.lib.mg_workspace_bytes(eng.model, B, L, 1, 0, T, 0, C.byref(need)) == 0
        assert need.value == nbytes, (B, L, T, need.value, nbytes)
        if T > 0:
            base = need.value
            assert eng.lib.mg_score_workspace_bytes(eng.model, B, L, T, 0, C.byref(need)) == 0
            # the teacher-forced layout plus 16 bytes per position (rows padded to 32) and 1024-column slab, plus the error word
            slabs = (shape.vocab_size + 1023) // 1024
            assert base < need.value <= base + 256 + slabs * ((B * T + 31) // 32 * 32) * 16 + 256


@pytest.mark.parametrize("be_name", BACKENDS)
def test_candidates_and_generated_ids(be_name):
    g, shape, eng, args, labels, dec = _case(be_name, "g3_trained_tiny.npz")
    T = int(g["max_length"])
    ids, _, _, ex = eng.generate(*args, num_beams=1, max_length=T, return_scores=True)
    ids, ts = _np(eng, ids).copy(), _np(eng, ex["token_scores"]).copy()
    tok, arg, _ = (_np(eng, a) for a in eng.score(*args, ids[:, :-1], ids[:, 1:]))
    live = np.zeros_like(ts, dtype=bool)
    for b, r in enumerate(ids):
        e = np.flatnonzero(r[1:] == shape.eos_token_id)
        live[b, :(e[0] + 1 if len(e) else ts.shape[1])] = True
    print("generate() token scores vs score(): max abs difference", np.abs(ts - tok)[live].max())
    assert np.abs(ts - tok)[live].max() < TOL
    assert np.array_equal(arg[live], ids[:, 1:][live])          # greedy ids are the teacher-forced argmax on the trained fixture
    # three candidates per image: the generated ids, the labels' first columns, a shuffled copy
    n = ids.shape[1] - 1
    lab = np.where(labels[:, :n] < 0, shape.pad_token_id, labels[:, :n])
    if lab.shape[1] < n:
        lab = np.concatenate([lab, np.full((lab.shape[0], n - lab.shape[1]), shape.pad_token_id, np.int64)], 1)
    cand = np.stack([ids[:, 1:], lab, np.roll(ids[:, 1:], 1, axis=0)], 1)
    cdec = np.concatenate([np.full(cand.shape[:2] + (1,), shape.decoder_start_token_id, np.int64), cand[..., :-1]], -1)
    tg = cand.copy()
    tg[:, 1, ::4] = -100                             # ignored positions in one candidate
    out = [_np(eng, a).copy() for a in eng.score_candidates(*args, cdec, tg)]
    assert out[0].shape == cand.shape and out[1].dtype == np.int64
    for c in range(3):
        one = [_np(eng, a) for a in eng.score(*args, cdec[:, c], tg[:, c])]
        for a, b in zip(out, one):
            assert np.ascontiguousarray(a[:, c]).tobytes() == np.ascontiguousarray(b).tobytes(), c
    assert np.all(out[0][:, 1, ::4] == 0.0)


@pytest.mark.parametrize("be_name", BACKENDS)
def test_errors(be_name):
    from markushgrapher_amd.engine import MgError
    g, shape, eng, args, labels, dec = _case(be_name, "g3_trained_tiny.npz")
    B, T = dec.shape
    mem, lib = eng.mem, eng.lib
    d_dec, d_tg = mem.asarray(dec, np.int64), mem.asarray(np.where(labels < 0, -100, labels), np.int64)
    tok = mem.empty((B, T), np.float32)

    def call(ws, nb, T_=T):
        return lib.mg_decoder_score(eng.model, mem.stream(), mem.ptr(ws), nb, mem.ptr(d_dec), None, mem.ptr(d_tg), B, T_, mem.ptr(tok), None, None)

    # no prior encode on this workspace
    need = C.c_size_t()
    assert lib.mg_score_workspace_bytes(eng.model, B, args[0].shape[1], T, 0, C.byref(need)) == 0
    ws = mem.empty((need.value,), np.uint8)
    assert call(ws, need.value) == MG_E_STATE
    # a target >= vocab (and the call after it is clean again: the error word is per call)
    bad = labels.copy()
    bad[0, 1] = shape.vocab_size
    with pytest.raises(MgError, match=f"error {MG_E_INPUT}: .*targets"):
        eng.score(*args, dec, bad)
    eng.score(*args, dec, labels)
    # T out of range (the engine of the tests decodes at most 64 positions)
    with pytest.raises(MgError, match=f"error {MG_E_SHAPE}:"):
        eng.score(*args, np.zeros((B, 65), np.int64), np.zeros((B, 65), np.int64))
    # a workspace sized for mg_decoder_forward only: too small for the partials
    eng.score(*args, dec, labels)                    # (leaves the encoder state of this batch in eng._ws)
    base = C.c_size_t()
    assert lib.mg_workspace_bytes(eng.model, B, args[0].shape[1], 1, 0, T, 0, C.byref(base)) == 0
    assert call(eng._ws, base.value) == MG_E_WORKSPACE
    assert call(eng._ws, eng._ws_bytes) == 0
