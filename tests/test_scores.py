"""Token log-probabilities and the beam n-best list (include/mgrapher.h mg_gen_opts; Engine.generate(return_scores=, num_return=);
model.generate(return_dict_in_generate=True, num_return_sequences=, output_scores=)).

  kernels   the lm_head epilogue's (max, sum) partials (TopOut::lse) and the fused / unfused greedy selection's token scores
  stock     tests/golden/scores_tiny.npz (tools/make_golden_scores.py): greedy compute_transition_scores(normalize_logits=True), beam-5
            n-best sequences / sequences_scores / beam_indices / transition scores, a min_length case and an early_stopping case
  G4        greedy token scores against the log-softmax of the teacher-forced logits (an independent code path), both cross-attention forms
  unchanged ids with scores on are bit-identical to the same call with scores off; hypothesis 0 of the n-best list is today's row

Tolerances: logit_tol (tests/test_engine.py) for the stock comparisons - a log-probability moves by at most twice the error of the logits
it is made of, the fixtures' logits are O(1); sequence scores are means of token log-probabilities and get the same bound."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import pkutil as pk
from tests.backends import get_backend, make_engine
from tests.conftest import load_golden
from tests.test_oracle_golden import _inputs, _weights

BACKENDS = [pytest.param("emu"), pytest.param("hip", marks=pytest.mark.gpu)]
TOL = 0.05          # 2 x logit_tol of the tiny fixtures (max |logit| ~ 1: 0.015 + 0.02 ~ 0.035 each side of the log-softmax)


def rnd(shape, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


def _log_softmax(x):
    m = x.max(-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))


def _lm_head(be, M, N, K, lse, eos):
    x, w = rnd((M, K), 11), rnd((N, K), 12, 0.3)
    X, W = be.buf(pk.pack_tiles(x)), be.buf(pk.pack_tiles(w))
    nt = (N + 31) // 32
    ldp = nt * 32
    P = be.zeros((M, ldp), np.float32)
    ptop, stopv = be.zeros((M, nt, 4), np.float32), be.zeros((M, 4), np.float32)
    assert be.lib.mgk_lm_head_top(be.stream, be.p(X), be.p(W), be.p(P), M, N, K, ldp, be.p(ptop), be.p(stopv), eos, lse) == 0
    return P.numpy()[:, :N].copy(), ptop.numpy().copy(), stopv.numpy().copy()


@pytest.mark.parametrize("be_name", BACKENDS)
def test_lm_head_lse_partials(be_name):
    """TopOut::lse: .x/.y/.z bit-equal to the flag off, .w = sum exp(x - .x) over the tile's non-stop features; the merged log-sum-exp
    within 1e-5 relative of numpy's on the same logits."""
    be = get_backend(be_name)
    M, N, K, eos = 40, 500, 128, 1
    lg0, p0, s0 = _lm_head(be, M, N, K, 0, eos)
    lg1, p1, s1 = _lm_head(be, M, N, K, 1, eos)
    assert np.array_equal(lg0, lg1) and np.array_equal(s0, s1)
    assert np.array_equal(p0[..., :3].view(np.int32), p1[..., :3].view(np.int32))
    assert np.all(p0[..., 3] == 0)
    x = lg1.astype(np.float64).copy()
    x[:, eos] = -np.inf                              # the stop token is kept apart (stopv)
    m, s = p1[..., 0].astype(np.float64), p1[..., 3].astype(np.float64)
    mx = m.max(-1, keepdims=True)
    lse = mx[:, 0] + np.log((s * np.exp(m - mx)).sum(-1))
    ref = np.log(np.exp(x - x.max(-1, keepdims=True)).sum(-1)) + x.max(-1)
    np.testing.assert_allclose(lse, ref, rtol=1e-5)
    assert np.array_equal(s1[:, 0], lg1[:, eos])


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("min_len", [0, 6])
def test_fused_and_unfused_selection_token_scores(be_name, min_len):
    """Both selection kernels write the same token scores (log_softmax of the processed logits at the chosen token): with EOS live and
    with EOS suppressed by MinLength, where it leaves the normaliser; a finished row writes 0."""
    be = get_backend(be_name)
    M, N, K, eos, max_len, pos = 40, 500, 128, 1, 8, 3
    lg, ptop, stopv = _lm_head(be, M, N, K, 1, eos)
    # make EOS the best token of a few rows (the fixture logits are random)
    unf = np.ones(M, np.int32)
    unf[5] = 0
    ldl = (N + 31) // 32 * 32
    L = np.full((M, ldl), -3.0e38, np.float32)
    L[:, :N] = lg
    res = []
    for fused in (False, True):
        nxt, out = be.zeros((M,), np.int64), be.zeros((M, max_len), np.int64)
        ub, nu, ts = be.buf(unf), be.zeros((1,), np.int32), be.zeros((M, max_len - 1), np.float32)
        if fused:
            d = 64
            emb, gain = rnd((N, d), 13), np.ones(d, np.float32)
            h, xpk = be.zeros((M, d), np.float32), be.zeros((((M + 31) // 32) * 32 * d,), np.uint16)
            rc = be.lib.mgk_greedy_select_fused(be.stream, be.p(be.buf(ptop)), be.p(be.buf(stopv)), M, N, eos, 0, min_len, be.p(nxt),
                                                be.p(out), max_len, pos, be.p(ub), be.p(nu), be.p(ts), max_len - 1,
                                                be.p(be.buf(pk.bf16_bits(emb))), be.p(be.buf(gain)), be.p(h), be.p(xpk), d, C.c_float(1e-6))
        else:
            rc = be.lib.mgk_greedy_select_scored(be.stream, be.p(be.buf(L)), M, N, ldl, eos, 0, min_len, be.p(nxt), be.p(out), max_len,
                                                 pos, be.p(ub), be.p(nu), be.p(ts), max_len - 1)
        assert rc == 0
        res.append((nxt.numpy().copy(), ts.numpy().copy()))
    (n0, t0), (n1, t1) = res
    assert np.array_equal(n0, n1)
    x = lg.astype(np.float64).copy()
    if pos < min_len:
        x[:, eos] = -np.inf
    ref = np.take_along_axis(_log_softmax(x), n0[:, None], -1)[:, 0]
    ref[unf == 0] = 0.0
    for t in (t0, t1):
        np.testing.assert_allclose(t[:, pos - 1], ref, rtol=1e-5, atol=1e-6)
        assert np.all(np.delete(t, pos - 1, axis=1) == 0)
    np.testing.assert_allclose(t0, t1, rtol=1e-5, atol=1e-6)


def _engine_case(be_name, fixture):
    g = load_golden(fixture)
    shape, sd = _weights(g)
    inp = _inputs(g, shape)
    eng = make_engine(be_name, shape, sd)
    return eng, (inp["input_ids"], inp["bbox"], inp["attention_mask"], inp["pixel_values"]), shape


def _np(eng, h):
    return eng.mem.numpy(h) if h is not None else None


def _check_greedy(eng, args, s, pre, case, shape, **kw):
    T = int(s["max_length"])
    ids, _, _, ex = eng.generate(*args, num_beams=1, max_length=T, return_scores=True, **kw)
    ids, ts = _np(eng, ids), _np(eng, ex["token_scores"])
    ref_ids, ref_ts = s[f"{pre}.{case}.sequences"], s[f"{pre}.{case}.transition_scores"]
    if pre == "g3":
        assert np.array_equal(ids, ref_ids)          # trained fixture: margins far above the noise
    # G0's near-tied steps may pick another token under bf16 noise (tests/test_engine.py pins its ids by margin): a token's score is
    # compared while the prefix it is scored on is stock's
    live = np.zeros_like(ts, dtype=bool)
    for b, r in enumerate(ids):
        e = np.flatnonzero(r[1:] == shape.eos_token_id)
        live[b, :(e[0] + 1 if len(e) else ts.shape[1])] = True
    same = np.zeros_like(live)
    for b in range(ids.shape[0]):
        n = min(ids.shape[1], ref_ids.shape[1])
        d = np.flatnonzero(ids[b, :n] != ref_ids[b, :n])
        same[b, :(d[0] - 1 if len(d) else n - 1)] = True
    assert same[:, 0].all()
    assert np.abs(ts - ref_ts[:, :ts.shape[1]])[live & same].max() < TOL
    assert np.all(ts[~live] == 0)                    # after a row's EOS: 0.0 (stock scores the pad token there)


def _pinned(ref_scores, K):
    """Hypotheses of stock's n-best list whose score is clear of both neighbours' by more than the noise (2 x TOL): which hypothesis holds
    that rank is decided, so its ids, beam indices and token scores are compared.  The last rank is never pinned (its lower neighbour,
    rank K + 1, is not in the list).  Everywhere else only the score of each rank is compared."""
    sc = ref_scores.reshape(-1, K).astype(np.float64)
    gap = np.full((sc.shape[0], K + 1), np.inf)
    gap[:, 1:K] = sc[:, :-1] - sc[:, 1:]
    gap[:, K] = 0.0
    return (np.minimum(gap[:, :K], gap[:, 1:]) > 2 * TOL).reshape(-1)


def _check_beam(eng, args, s, pre, case, **kw):
    T, K = int(s["max_length"]), int(s["num_beams"])
    ids, sc, _, ex = eng.generate(*args, num_beams=K, max_length=T, num_return=K, return_scores=True, **kw)
    ids, sc, ts, bi = _np(eng, ids), _np(eng, sc), _np(eng, ex["token_scores"]), _np(eng, ex["beam_indices"])
    ref_ids, ref_sc = s[f"{pre}.{case}.sequences"], s[f"{pre}.{case}.sequences_scores"]
    pin = _pinned(ref_sc, K)
    assert ids.shape[0] == ref_ids.shape[0]
    np.testing.assert_allclose(sc[::K], ref_sc[::K], atol=TOL)      # the best hypothesis' score, decided or not
    np.testing.assert_allclose(sc[pin], ref_sc[pin], atol=TOL)
    if pre == "g3" and case == "beam":
        assert pin[::K].all()                        # the trained fixture decides every image's best hypothesis
    for r in np.flatnonzero(pin):
        n = int((s[f"{pre}.{case}.beam_indices"][r] >= 0).sum())
        assert np.array_equal(ids[r, :n + 1], ref_ids[r, :n + 1]) and np.all(bi[r, n:] == -1)
        assert np.array_equal(bi[r, :n], s[f"{pre}.{case}.beam_indices"][r, :n])
        np.testing.assert_allclose(ts[r], s[f"{pre}.{case}.transition_scores"][r, :ts.shape[1]], atol=TOL)
    # stock's compute_transition_scores docstring: summed token scores / length ** length_penalty = sequences_scores
    lp = kw.get("length_penalty", 1.0)
    n = (bi >= 0).sum(1)
    np.testing.assert_allclose(ts.sum(1) / n.astype(np.float64) ** lp, sc, rtol=1e-5, atol=1e-6)
    return ids, sc


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("fixture,pre", [("g3_trained_tiny.npz", "g3"), ("g0_tiny.npz", "g0")])
def test_scores_match_stock(be_name, fixture, pre):
    if be_name == "emu" and pre != "g3":
        pytest.skip("one fixture is enough on the emulator")
    s = load_golden("scores_tiny.npz")
    eng, args, shape = _engine_case(be_name, fixture)
    _check_greedy(eng, args, s, pre, "greedy", shape)
    _check_greedy(eng, args, s, pre, "greedy_min", shape, min_length=int(s["min_length"]))
    T, K = int(s["max_length"]), int(s["num_beams"])
    ids, sc = _check_beam(eng, args, s, pre, "beam")
    # hypothesis 0 of the n-best list is the unscored call's row and score
    b_ids, b_sc, _ = eng.generate(*args, num_beams=K, max_length=T)
    b_ids, b_sc = _np(eng, b_ids), _np(eng, b_sc)
    assert np.array_equal(ids[::K, :b_ids.shape[1]], b_ids) and np.all(ids[::K, b_ids.shape[1]:] == (shape.pad_token_id or shape.eos_token_id))
    assert np.array_equal(sc[::K], b_sc)
    _check_beam(eng, args, s, pre, "beam_es", early_stopping=True, length_penalty=0.7)


@pytest.mark.parametrize("be_name", BACKENDS)
def test_scores_leave_ids_unchanged(be_name):
    """Scores on: ids bit-identical to the same call with scores off (greedy batch through graph replay, greedy queue, beam batch, beam
    queue), and the queue's per-image token scores equal the batch call's."""
    eng, args, shape = _engine_case(be_name, "g3_trained_tiny.npz")
    T = 16
    for _ in range(2):                               # the second round replays the graphs captured by the first
        off, _, _ = eng.generate(*args, max_length=T)
        on, _, _, ex = eng.generate(*args, max_length=T, return_scores=True)
        assert np.array_equal(_np(eng, off), _np(eng, on))
        ts = _np(eng, ex["token_scores"])
        for K in (3, 5):
            off, osc, _ = eng.generate(*args, num_beams=K, max_length=T)
            on, sc, _, _ = eng.generate(*args, num_beams=K, max_length=T, return_scores=True)
            assert np.array_equal(_np(eng, off), _np(eng, on)) and np.array_equal(_np(eng, osc), _np(eng, sc))
    N = args[0].shape[0]
    prev = eng.set_padding_semantics(True)
    try:
        q_off = eng.generate_stream(*args, max_length=T, chunk=3, slots=2)
        q_on = eng.generate_stream(*args, max_length=T, chunk=3, slots=2, return_scores=True)
        assert np.array_equal(_np(eng, q_off[0]), _np(eng, q_on[0])) and np.array_equal(_np(eng, q_off[1]), _np(eng, q_on[1]))
        qts, qlen = _np(eng, q_on[3]), _np(eng, q_on[1])
        for i in range(N):
            one = tuple(a[i:i + 1] if a is not None else None for a in args)
            _, _, _, ex1 = eng.generate(*one, max_length=T, return_scores=True)
            t1 = _np(eng, ex1["token_scores"])[0]
            # (the queue selects with the full-row scan, the batch call with the fused tail: the normaliser is summed in another order)
            np.testing.assert_allclose(qts[i, :len(t1)], t1, rtol=1e-5, atol=1e-6)
            assert np.all(qts[i, qlen[i] - 1:] == 0)
        K = 5
        b_off = eng.generate_stream_beam(*args, num_beams=K, max_length=T, chunk=3, slots=2)
        b_on = eng.generate_stream_beam(*args, num_beams=K, max_length=T, chunk=3, slots=2, num_return=K, return_scores=True)
        ids_on = _np(eng, b_on[0])
        assert np.array_equal(_np(eng, b_off[0]), ids_on[::K]) and np.array_equal(_np(eng, b_off[2]), _np(eng, b_on[2])[::K])
        for i in range(N):
            one = tuple(a[i:i + 1] if a is not None else None for a in args)
            ids1, sc1, _, ex1 = eng.generate(*one, num_beams=K, max_length=T, num_return=K, return_scores=True)
            ids1 = _np(eng, ids1)
            assert np.array_equal(ids_on[i * K:(i + 1) * K, :ids1.shape[1]], ids1)
            np.testing.assert_array_equal(_np(eng, b_on[2])[i * K:(i + 1) * K], _np(eng, sc1))
            n = ids1.shape[1] - 1
            np.testing.assert_array_equal(_np(eng, b_on[4]["token_scores"])[i * K:(i + 1) * K, :n], _np(eng, ex1["token_scores"]))
            bi = _np(eng, b_on[4]["beam_indices"])[i * K:(i + 1) * K, :n]
            np.testing.assert_array_equal(np.where(bi >= 0, bi - i * K, bi), _np(eng, ex1["beam_indices"]))
    finally:
        eng.set_padding_semantics(prev)


def test_num_return_is_validated():
    eng, args, _ = _engine_case("emu", "g3_trained_tiny.npz")
    with pytest.raises(ValueError):
        eng.generate(*args, num_beams=1, max_length=8, num_return=2)
    with pytest.raises(ValueError):
        eng.generate(*args, num_beams=3, max_length=8, num_return=4)


# ---- HF surface (model.generate / compute_transition_scores / generate_queue), GPU --------------------------------------------------

def _model_and_inputs(fixture):
    from tests.test_modeling import tiny_model
    from markushgrapher_amd import synth
    g = load_golden(fixture)
    m, shape = tiny_model()
    if "recipe" in g:
        _, sd = _weights(g)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in {**sd, **{a: sd[c] for a, c in synth.tied_aliases(shape).items()}}.items()})
    m = m.to("cuda")
    kw = {k: torch.from_numpy(np.asarray(v)).to(m.device) for k, v in _inputs(g, shape).items()}
    return m, kw


@pytest.mark.gpu
def test_hf_generate_n_best_dict():
    s = load_golden("scores_tiny.npz")
    m, kw = _model_and_inputs("g3_trained_tiny.npz")
    T, K = int(s["max_length"]), int(s["num_beams"])
    B = kw["input_ids"].shape[0]
    out = m.generate(**kw, num_beams=K, num_return_sequences=K, max_length=T, return_dict_in_generate=True)
    assert out.sequences.shape[0] == B * K and out.beam_indices.shape[1] == out.sequences.shape[1] - 1
    pin = _pinned(s["g3.beam.sequences_scores"], K)
    np.testing.assert_allclose(out.sequences_scores.cpu().numpy()[pin], s["g3.beam.sequences_scores"][pin], atol=TOL)
    assert pin[::K].all()                            # every image's best hypothesis is decided
    seq, ref = out.sequences.cpu().numpy(), s["g3.beam.sequences"]
    for r in np.flatnonzero(pin):
        n = int((s["g3.beam.beam_indices"][r] >= 0).sum())
        assert np.array_equal(seq[r, :n + 1], ref[r, :n + 1])
        assert np.array_equal(out.beam_indices[r, :n].cpu().numpy(), s["g3.beam.beam_indices"][r, :n])
        np.testing.assert_allclose(out.token_scores[r, :n].cpu().numpy(), s["g3.beam.transition_scores"][r, :n], atol=TOL)
    ids = m.generate(**kw, num_beams=K, num_return_sequences=K, max_length=T)
    assert torch.equal(ids, out.sequences)
    assert torch.equal(m.generate(**kw, num_beams=K, max_length=T), out.sequences[::K, :m.generate(**kw, num_beams=K, max_length=T).shape[1]])
    g = m.generate(**kw, max_length=T, return_dict_in_generate=True)
    assert g.sequences_scores is None and g.beam_indices is None and g.scores is None
    assert torch.equal(g.sequences, m.generate(**kw, max_length=T))
    with pytest.raises(ValueError):
        m.generate(**kw, num_beams=3, num_return_sequences=5, max_length=T)
    with pytest.raises(ValueError):
        m.generate(**kw, num_return_sequences=2, max_length=T)


@pytest.mark.gpu
def test_hf_output_scores_and_compute_transition_scores():
    """output_scores / output_logits (full vocabulary, through the decode-capture instrumentation): G0's stored stock scores, and
    compute_transition_scores on them reproduces the fixture and the device token scores."""
    s = load_golden("scores_tiny.npz")
    m, kw = _model_and_inputs("g0_tiny.npz")
    T, K = int(s["max_length"]), int(s["num_beams"])
    g = m.generate(**kw, max_length=T, return_dict_in_generate=True, output_scores=True, output_logits=True)
    seq = g.sequences.cpu().numpy()
    assert torch.equal(g.sequences, m.generate(**kw, max_length=T))
    sc = torch.stack(g.scores, 1).cpu().numpy()
    tr = m.compute_transition_scores(g.sequences, g.scores, normalize_logits=True).cpu().numpy()
    for b in range(seq.shape[0]):                    # while the row's prefix is stock's (G0 has near-tied steps; see _check_greedy)
        d = np.flatnonzero(seq[b] != s["g0.greedy.sequences"][b])
        n = d[0] if len(d) else seq.shape[1] - 1
        assert n >= 1
        np.testing.assert_allclose(sc[b, :n], s["g0.greedy.scores"][b, :n], atol=TOL)
        np.testing.assert_allclose(tr[b, :n - 1 if len(d) else n], s["g0.greedy.transition_scores"][b, :n - 1 if len(d) else n], atol=TOL)
    assert all(torch.equal(a, b) for a, b in zip(g.scores, g.logits))     # greedy, min_length 0: processed = raw
    np.testing.assert_allclose(tr, g.token_scores.cpu().numpy(), atol=1e-4)
    b = m.generate(**kw, num_beams=K, num_return_sequences=K, max_length=T, return_dict_in_generate=True, output_scores=True)
    # G0's hypotheses are near-tied (gaps of 1e-3): which beams run after the first step is not decided under bf16 noise, the first
    # step's scores (every beam of an image fed the start token) are
    np.testing.assert_allclose(b.scores[0].cpu().numpy(), s["g0.beam.scores"][:, 0], atol=TOL)
    assert len(b.scores) == b.sequences.shape[1] - 1 and b.scores[0].shape == (kw["input_ids"].shape[0] * K, 500)
    tr = m.compute_transition_scores(b.sequences, b.scores, b.beam_indices, normalize_logits=False).cpu().numpy()
    np.testing.assert_allclose(tr, b.token_scores.cpu().numpy(), atol=1e-5)
    n = (b.beam_indices >= 0).sum(1).cpu().numpy()
    np.testing.assert_allclose(tr.sum(1) / n, b.sequences_scores.cpu().numpy(), rtol=1e-5, atol=1e-6)
    gm = m.generate(**kw, max_length=T, min_length=int(s["min_length"]), return_dict_in_generate=True, output_scores=True)
    eos = m.config.eos_token_id
    assert all(torch.isinf(gm.scores[t][:, eos]).all() for t in range(int(s["min_length"]) - 1))
    tr = m.compute_transition_scores(gm.sequences, gm.scores, normalize_logits=True).cpu().numpy()
    np.testing.assert_allclose(tr, gm.token_scores.cpu().numpy(), atol=1e-4)


@pytest.mark.gpu
def test_hf_generate_queue_scores():
    m, kw = _model_and_inputs("g3_trained_tiny.npz")
    T = 16
    enc = [dict(input_ids=kw["input_ids"][i:i + 1], bbox=kw["bbox"][i:i + 1], pixel_values=kw["pixel_values"][i:i + 1])
           for i in range(kw["input_ids"].shape[0])]
    plain = m.generate_queue(enc, max_length=T, slots=3, chunk=3)
    rows = m.generate_queue(enc, max_length=T, slots=3, chunk=3, return_scores=True)
    beams = m.generate_queue(enc, max_length=T, slots=3, chunk=3, num_beams=5, num_return_sequences=5, return_scores=True)
    for i, (p, r, b) in enumerate(zip(plain, rows, beams)):
        assert torch.equal(r["sequences"][0], p)
        # generate() of one image and the queue (per-image padding semantics) give the same ids, their logits agree within the noise
        one = m.generate(**enc[i], max_length=T, return_dict_in_generate=True)
        assert torch.equal(r["sequences"], one.sequences)
        torch.testing.assert_close(r["token_scores"], one.token_scores, atol=TOL, rtol=0)
        ob = m.generate(**enc[i], num_beams=5, num_return_sequences=5, max_length=T, return_dict_in_generate=True)
        assert b["sequences"].shape[0] == 5 and b["beam_indices"].shape == b["token_scores"].shape == (5, b["sequences"].shape[1] - 1)
        w = min(b["sequences"].shape[1], ob.sequences.shape[1])
        assert torch.equal(b["sequences"][0, :w], ob.sequences[0, :w])
        torch.testing.assert_close(b["sequences_scores"][0], ob.sequences_scores[0], atol=TOL, rtol=0)
        n = (b["beam_indices"] >= 0).sum(1)
        torch.testing.assert_close(b["token_scores"].sum(1) / n, b["sequences_scores"], atol=1e-6, rtol=1e-5)


# ---- large shape: greedy token scores against the teacher-forced forward, GPU -------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("absorb", [False, True])
def test_g4_token_scores_vs_teacher_forced(absorb):
    from tests.test_bench_config import LOGIT_TOL, _setup
    g, shape, eng, args = _setup()
    eng.set_cross_absorb(absorb)
    try:
        ids, _, _, ex = eng.generate(*args, max_length=17, return_scores=True)
        ids, ts = eng.mem.numpy(ids), eng.mem.numpy(ex["token_scores"])
        logits, _, _ = eng.forward_logits(*args, ids[:, :-1])
        lp = _log_softmax(eng.mem.numpy(logits).astype(np.float64))
        ref = np.take_along_axis(lp, ids[:, 1:, None], -1)[..., 0]
    finally:
        eng.set_cross_absorb(True)                   # _setup's setting
    live = np.ones_like(ref, dtype=bool)
    for b, r in enumerate(ids):
        e = np.flatnonzero(r[1:] == shape.eos_token_id)
        if len(e):
            live[b, e[0] + 1:] = False
    assert np.abs(ts - ref)[live].max() < 2 * LOGIT_TOL
    assert np.all(ts[~live] == 0)
