"""On-device sampling, engine level: mg_generate_sampled through Engine.generate_sampled (include/mgrapher.h mg_sample_opts) on the
trained-tiny fixture G3 and the tiny random model G0.

  greedy-equivalent   top_k = 1 ids equal generate(num_beams = 1), eager / captured graph / eager device-counter form
  graph key           seed A, seed B, seed A, other temperatures, with and without token scores on one engine: nothing stale
  call size           a batch alone = the same batch as the first rows of a 64-row call (same stream ids, cross-attention form pinned)
  num_return = 4      row b * 4 + j = row b of a one-sample call whose stream id is that row's; one encoder pass
  scores              pure temperature sampling: token_scores = log_softmax(teacher-forced logits / T) at the emitted tokens
"""
import ctypes as C

import numpy as np
import pytest

from markushgrapher_amd.engine import MgError
from tests.backends import make_engine
from tests.conftest import load_golden
from tests.test_oracle_golden import _inputs, _weights
from tests.test_scores import TOL, _log_softmax

BACKENDS = [pytest.param("emu"), pytest.param("hip", marks=pytest.mark.gpu)]
FIXTURES = ["g3_trained_tiny.npz", "g0_tiny.npz"]


def _case(be_name, fixture):
    g = load_golden(fixture)
    shape, sd = _weights(g)
    inp = _inputs(g, shape)
    eng = make_engine(be_name, shape, sd)
    T = int(g["max_length"]) if "max_length" in g else 16
    return eng, (inp["input_ids"], inp["bbox"], inp["attention_mask"], inp["pixel_values"]), shape, min(T, 24)


def _np(eng, h):
    return np.array(eng.mem.numpy(h), copy=True)


def _sample(eng, args, **kw):
    ids, cols, ts = eng.generate_sampled(*args, **kw)
    return _np(eng, ids), (_np(eng, ts) if ts is not None else None)


def _pad_to(a, cols, pad):
    out = np.full((a.shape[0], cols), pad, a.dtype)
    out[:, :a.shape[1]] = a
    return out


def _same_ids(a, b, pad):
    """Two id matrices that may differ in the number of (pad) columns the call returned."""
    n = max(a.shape[1], b.shape[1])
    return np.array_equal(_pad_to(a, n, pad), _pad_to(b, n, pad))


def _absorb_settings(eng):
    out = [False]
    try:
        eng.set_cross_absorb(True)
        out.append(True)
    except MgError:
        pass
    eng.set_cross_absorb("auto")
    return out


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("fixture", FIXTURES)
def test_top_k_1_equals_greedy(be_name, fixture):
    eng, args, shape, T = _case(be_name, fixture)
    ref, _, _ = eng.generate(*args, num_beams=1, max_length=T)
    ref = _np(eng, ref)
    for mode in ((0, 2) if be_name == "emu" else (1, 0, 2)):
        eng.set_decode_graph(mode)
        try:
            for seed in (1, 2):
                ids, ts = _sample(eng, args, max_length=T, top_k=1, temperature=0.7, seed=seed, return_scores=True)
                assert np.array_equal(ids, ref), (mode, seed)
                assert np.all(ts == 0.0)
            if mode == 1:
                assert eng.decode_graph_active()
            ids, _ = _sample(eng, args, max_length=T, top_k=0, top_p=1e-6, seed=3)
            assert np.array_equal(ids, ref), (mode, "top_p")
        finally:
            eng.set_decode_graph(1)


@pytest.mark.parametrize("be_name", BACKENDS)
def test_graph_key_holds_every_sampling_parameter(be_name):
    """Back-to-back calls on one engine (hip: the captured step is replayed or re-captured by its key)."""
    eng, args, shape, T = _case(be_name, "g0_tiny.npz")
    kw = dict(max_length=T, min_length=T, temperature=1.5, top_k=0, top_p=1.0)      # no early stop: every column is a draw
    a1, _ = _sample(eng, args, seed=101, **kw)
    b1, _ = _sample(eng, args, seed=202, **kw)
    a2, _ = _sample(eng, args, seed=101, **kw)
    assert np.array_equal(a1, a2)
    assert not np.array_equal(a1, b1)
    a3, ts3 = _sample(eng, args, seed=101, return_scores=True, **kw)
    assert np.array_equal(a1, a3) and np.all(ts3 < 0)
    a4, _ = _sample(eng, args, seed=101, **kw)
    assert np.array_equal(a1, a4)
    # temperature, top_k, top_p and the stream ids are held by the captured launch, too
    g, _, _ = eng.generate(*args, num_beams=1, max_length=T, min_length=T)
    g = _np(eng, g)
    cold, _ = _sample(eng, args, seed=101, **dict(kw, temperature=0.3))
    assert not np.array_equal(cold, a1), "another temperature, other draws from the same random numbers"
    k1, _ = _sample(eng, args, seed=101, **dict(kw, top_k=1))
    assert np.array_equal(k1, g)
    p0, _ = _sample(eng, args, seed=101, **dict(kw, top_p=1e-6))
    assert np.array_equal(p0, g)
    a5, _ = _sample(eng, args, seed=101, **kw)
    assert np.array_equal(a1, a5)
    B = a1.shape[0]
    s1, _ = _sample(eng, args, seed=101, stream_ids=np.arange(B) + 1000, **kw)
    assert not np.array_equal(s1, a1)
    s0, _ = _sample(eng, args, seed=101, stream_ids=np.arange(B), **kw)
    assert np.array_equal(s0, a1), "default stream ids are the row indices"
    # greedy and beam calls in between are unaffected and leave nothing behind
    g2, _, _ = eng.generate(*args, num_beams=1, max_length=T, min_length=T)
    assert np.array_equal(_np(eng, g2), g)
    a6, _ = _sample(eng, args, seed=101, **kw)
    assert np.array_equal(a1, a6)


@pytest.mark.parametrize("be_name", BACKENDS)
def test_call_size_independence(be_name):
    eng, args, shape, T = _case(be_name, "g0_tiny.npz")
    T = min(T, 10)
    B = args[0].shape[0]
    reps = 64 // B
    big = tuple(np.concatenate([a] * reps, 0) for a in args)
    sid_big = np.arange(B * reps) * 7 + 3
    kw = dict(max_length=T, min_length=T, temperature=1.3, top_k=20, top_p=0.95, seed=77)
    for absorb in _absorb_settings(eng):
        eng.set_cross_absorb(absorb)
        try:
            small, _ = _sample(eng, args, stream_ids=sid_big[:B], **kw)
            large, _ = _sample(eng, big, stream_ids=sid_big, **kw)
            assert np.array_equal(small, large[:B]), absorb
            assert not np.array_equal(large[:B], large[B:2 * B]), "other stream ids, other draws"
        finally:
            eng.set_cross_absorb("auto")


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("fixture", FIXTURES)
def test_num_return_4_rows_are_independent_samples(be_name, fixture):
    eng, args, shape, T = _case(be_name, fixture)
    T = min(T, 12)
    B = args[0].shape[0]
    sid = np.arange(B * 4) * 13 + 1
    kw = dict(max_length=T, temperature=1.4, top_k=0, top_p=0.98, seed=5)
    for absorb in _absorb_settings(eng):
        eng.set_cross_absorb(absorb)
        try:
            four, ts4 = _sample(eng, args, num_return=4, stream_ids=sid, return_scores=True, **kw)
            assert four.shape[0] == B * 4
            for j in range(4):
                one, ts1 = _sample(eng, args, num_return=1, stream_ids=sid[j::4], return_scores=True, **kw)
                assert _same_ids(four[j::4], one, shape.pad_token_id), (absorb, j)
                n = min(ts4.shape[1], ts1.shape[1])
                assert np.array_equal(ts4[j::4, :n], ts1[:, :n])
            if fixture == "g0_tiny.npz":
                assert not np.array_equal(four[0::4], four[1::4]), "the samples of an image differ"
        finally:
            eng.set_cross_absorb("auto")


def test_num_return_runs_the_encoder_once_per_image():
    """The emulator counts the workgroups it executes.  A call that samples 4 rows per image must launch the encoder (and the cross
    K/V projections) over B images, not over 4 B rows: its workgroups stay below those of a one-sample call on the images replicated 4
    times by at least the encoder's own difference between 4 B and B images.  One decode step, so the decode launches of the two calls
    (same 4 B rows) are alike."""
    eng, args, shape, _ = _case("emu", "g0_tiny.npz")
    eng.lib.emu_workgroups_launched.restype = C.c_long
    B = args[0].shape[0]
    rep4 = tuple(np.concatenate([a] * 4, 0) for a in args)

    def work(fn):
        w0 = eng.lib.emu_workgroups_launched()
        fn()
        return eng.lib.emu_workgroups_launched() - w0

    eng.set_cross_absorb(False)
    try:
        enc_b = work(lambda: eng.encode(*args, want_out=False))
        enc_4b = work(lambda: eng.encode(*rep4, want_out=False))
        assert enc_4b > enc_b
        kw = dict(max_length=2, min_length=2, temperature=1.2, seed=1)
        shared = work(lambda: eng.generate_sampled(*args, num_return=4, **kw))
        replicated = work(lambda: eng.generate_sampled(*rep4, num_return=1, **kw))
        print(f"workgroups: encoder {enc_b} (B images) / {enc_4b} (4 B); sampled call {shared} (num_return = 4) / {replicated} (4 B images)")
        assert shared <= replicated - (enc_4b - enc_b)
    finally:
        eng.set_cross_absorb("auto")


@pytest.mark.parametrize("be_name", BACKENDS)
def test_top2_record_of_live_rows_is_greedy_selects(be_name):
    """step_top2 under sampling: rows that are live at a step hold the top-2 of their logits as the greedy call records them (top_k = 1
    follows the greedy path exactly); rows finished before the step hold 0 - the sampled selection does not read a finished row."""
    eng, args, shape, T = _case(be_name, "g3_trained_tiny.npz")
    ref, _, top_g = eng.generate(*args, num_beams=1, max_length=T, return_top2=True)
    ids, cols, _, top_s = eng.generate_sampled(*args, max_length=T, top_k=1, seed=1, return_top2=True)
    ref, ids, top_g, top_s = _np(eng, ref), _np(eng, ids), _np(eng, top_g), _np(eng, top_s)
    assert np.array_equal(ref, ids)
    seen_finished = False
    for b, r in enumerate(ids):
        e = np.flatnonzero(r[1:] == shape.eos_token_id)
        last = e[0] + 1 if len(e) else ids.shape[1] - 1          # last column the row itself selects
        np.testing.assert_allclose(top_s[1:last + 1, b], top_g[1:last + 1, b], rtol=0, atol=2e-2)
        assert np.all(top_s[1:last + 1, b, 0] > top_s[1:last + 1, b, 1])
        if last + 1 < cols:
            seen_finished = True
            assert np.all(top_s[last + 1:cols, b] == 0)
    assert seen_finished, "the fixture has rows that finish before the call ends"


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("fixture", FIXTURES)
@pytest.mark.parametrize("temperature", [1.0, 1.25])
def test_token_scores_vs_teacher_forced(be_name, fixture, temperature):
    eng, args, shape, T = _case(be_name, fixture)
    ids, ts = _sample(eng, args, max_length=T, temperature=temperature, top_k=0, top_p=1.0, seed=9, return_scores=True)
    logits, _, _ = eng.forward_logits(*args, ids[:, :-1])
    lp = _log_softmax(_np(eng, logits).astype(np.float64) / temperature)
    ref = np.take_along_axis(lp, ids[:, 1:, None], -1)[..., 0]
    live = np.ones_like(ref, dtype=bool)
    for b, r in enumerate(ids):
        e = np.flatnonzero(r[1:] == shape.eos_token_id)
        if len(e):
            live[b, e[0] + 1:] = False
    print(f"max |token score - teacher-forced| = {np.abs(ts - ref)[live].max():.4f} (bound {TOL})")
    assert np.abs(ts - ref)[live].max() < TOL
    assert np.all(ts[~live] == 0)


def test_arguments_are_validated():
    eng, args, shape, T = _case("emu", "g3_trained_tiny.npz")
    with pytest.raises(ValueError):
        eng.generate_sampled(*args, max_length=T, temperature=0.0)
    with pytest.raises(ValueError):
        eng.generate_sampled(*args, max_length=T, top_k=-1)
    with pytest.raises(ValueError):
        eng.generate_sampled(*args, max_length=T, top_p=0.0)
    with pytest.raises(ValueError):
        eng.generate_sampled(*args, max_length=T, num_return=0)
    with pytest.raises(MgError):
        eng.generate_sampled(*args, max_length=T, num_return=200)
    with pytest.raises(ValueError):
        eng.generate_sampled(*args, max_length=T, stream_ids=[1])
    # forced ids of the parity instrumentation are not built for sampling; the logits capture is
    B = args[0].shape[0]
    eng.debug_decode_capture(capture_steps=2, rows=B, forced_ids=np.zeros((B, T), np.int64))
    with pytest.raises(MgError):
        eng.generate_sampled(*args, max_length=T)
    cap = eng.debug_decode_capture(capture_steps=2, rows=B)
    ids, _, ts = eng.generate_sampled(*args, max_length=T, temperature=1.0, seed=4, return_scores=True)
    eng.debug_decode_capture()
    ids, ts, cap = _np(eng, ids), _np(eng, ts), _np(eng, cap)
    lp = _log_softmax(cap.astype(np.float64))
    for t in range(2):
        np.testing.assert_allclose(ts[:, t], np.take_along_axis(lp[t], ids[:, t + 1, None], -1)[:, 0], atol=1e-4)
