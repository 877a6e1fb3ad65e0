"""The greedy queue under sampling (C ABI mg_generate_stream_sampled through Engine.generate_stream_sampled): a queue of N images with S
samples each is a queue of N * S sequences on `slots` decode rows.  A row's draw depends on (seed, stream id, column, its own logits) and
the stream id of sequence q is q - its place in the queue, never its slot - so everything here is an EQUALITY with one-image batch calls
(Engine.generate_sampled on that image alone, stream id q), not a statistic.  `emu` = the same sources on the CPU SIMT emulator, `hip` =
MI355X (the step is a captured graph there).

  queue = per-image calls   three (chunk, slots, pool_chunks), both cross-attention forms; the parameter sets agree bit for bit
  num_return = 3            the samples of an image in different slots at different times while pool entries are recycled
  greedy-equivalent         top_k = 1 / top_p = 1e-6: generate_stream's ids and lengths, scores exactly 0
  forced length + scores    token scores equal the batch calls'; queues smaller than the slot count
  graph key                 every sampling option, num_return and the stream-id / score pointers; greedy and beam queues in between
  bad arguments             each names its argument; the engine still works afterwards
"""
import numpy as np
import pytest

from markushgrapher_amd.engine import MgError
from tests.backends import make_engine
from tests.conftest import load_golden
from tests.test_oracle_golden import _inputs, _weights

BACKENDS = [pytest.param("emu"), pytest.param("hip", marks=pytest.mark.gpu)]
ORDER = np.array([0, 3, 5, 1, 2, 4, 4, 0, 1, 5, 2, 3, 3, 0])      # 14 images in the queue (no chunk below divides it)
KEYS = ("input_ids", "bbox", "attention_mask", "pixel_values")
TEMP = 1.5      # see test_queue_equals_per_image_calls
SEED = 20261


def _np(eng, h):
    return np.array(eng.mem.numpy(h), copy=True)


def _case(be_name, fixture="g3_trained_tiny.npz"):
    g = load_golden(fixture)
    shape, sd = _weights(g)
    inp = _inputs(g, shape)
    eng = make_engine(be_name, shape, sd)
    T = int(g["max_length"]) if "max_length" in g else 16
    return eng, inp, shape, min(T, 24), g


def _args(inp, order):
    return tuple(np.ascontiguousarray(inp[k][np.asarray(order)]) for k in KEYS)


def _absorb_settings(eng):
    out = [False]
    try:
        eng.set_cross_absorb(True)
        out.append(True)
    except MgError:
        pass
    eng.set_cross_absorb("auto")
    return out


def _one_image(eng, inp, b, sid, shape, T, **kw):
    """generate_sampled on image b alone with stream id sid -> (row padded to T, length, token scores padded to T - 1)."""
    ids, cols, ts = eng.generate_sampled(*_args(inp, [b]), stream_ids=[sid], return_scores=True, max_length=T, **kw)
    ids, ts = _np(eng, ids)[0], _np(eng, ts)[0]
    e = np.flatnonzero(ids[1:] == shape.eos_token_id)
    n = int(e[0]) + 2 if len(e) else T
    assert n == cols or (len(e) == 0 and cols == T), (n, cols)
    row = np.full(T, shape.pad_token_id, ids.dtype)
    row[:n] = ids[:n]
    sc = np.zeros(T - 1, np.float32)
    sc[:n - 1] = ts[:n - 1]
    return row, n, sc


def _check_rows(ids, lens, want, shape):
    for q, (row, n, _) in enumerate(want):
        assert lens[q] == n, (q, lens[q], n)
        assert np.array_equal(ids[q, :n], row[:n]), (q, ids[q].tolist(), row.tolist())
        assert np.all(ids[q, n:] == shape.pad_token_id), q


@pytest.mark.parametrize("be_name", BACKENDS)
def test_queue_equals_per_image_calls(be_name):
    """Sequence n of the queue = the one-image call on image ORDER[n] with stream id n, for three slot geometries and both cross-attention
    forms (pinned: the default picks the form by the call's decode rows).
    Temperature: the lowest of 1.0 / 1.5 / 2.0 at which the per-image reference calls alone (emulator, K / V form, top_k = 0, top_p = 1,
    seed 20261) meet the three conditions asserted below.  Observed: T = 1.0 - 1 of 14 rows differs from greedy (fails the first
    condition); T = 1.5 - 11 of 14 differ from greedy, lengths 4 .. 16, 10 of the 11 duplicate pairs differ -> 1.5."""
    eng, inp, shape, T, g = _case(be_name)
    kw = dict(temperature=TEMP, top_k=0, top_p=1.0, seed=SEED)
    q = _args(inp, ORDER)
    for absorb in _absorb_settings(eng):
        eng.set_cross_absorb(absorb)
        try:
            want = [_one_image(eng, inp, b, n, shape, T, **kw) for n, b in enumerate(ORDER)]
            # the test is not vacuous: sampling moves the rows, the rows end at different steps, the random stream (not the image) names the draw
            greedy = g["greedy_ids"]
            differ = sum(1 for n, b in enumerate(ORDER) if not np.array_equal(want[n][0], _pad(greedy[b], shape, T)))
            dup = sum(1 for i in range(len(ORDER)) for j in range(i + 1, len(ORDER))
                      if ORDER[i] == ORDER[j] and not np.array_equal(want[i][0], want[j][0]))
            print(f"absorb {absorb}: {differ} of {len(ORDER)} rows differ from greedy, lengths {[w[1] for w in want]}, {dup} duplicate pairs differ")
            assert differ * 2 >= len(ORDER)
            assert len(set(w[1] for w in want)) > 1
            assert dup >= 1
            outs = []
            for chunk, slots, pool_chunks in ((4, 3, 2), (3, 5, 3), (6, 2, 2)):
                ids, lens, steps = eng.generate_stream_sampled(*q, max_length=T, chunk=chunk, slots=slots, pool_chunks=pool_chunks, **kw)
                ids, lens = _np(eng, ids), _np(eng, lens)
                _check_rows(ids, lens, want, shape)
                outs.append((ids, lens))
            for ids, lens in outs[1:]:      # slot placement changes nothing
                assert np.array_equal(ids, outs[0][0]) and np.array_equal(lens, outs[0][1])
        finally:
            eng.set_cross_absorb("auto")


def _pad(row, shape, T):
    """A golden greedy row in the queue's layout: cut after its EOS, padded to T."""
    e = np.flatnonzero(row == shape.eos_token_id)
    n = int(e[0]) + 1 if len(e) else len(row)
    out = np.full(T, shape.pad_token_id, row.dtype)
    out[:n] = row[:n]
    return out


@pytest.mark.parametrize("be_name", BACKENDS)
def test_num_return_3_shares_the_image_and_not_the_stream(be_name):
    """7 images x 3 samples on 5 slots, chunks of 2, 6 pool entries: the samples of an image sit in different slots at different times, and
    entries are overwritten while later images are still being sampled.  Row n * 3 + j = the one-image, one-sample call with stream id
    n * 3 + j."""
    eng, inp, shape, T, g = _case(be_name)
    eng.set_cross_absorb(False)
    try:
        kw = dict(temperature=TEMP, top_k=0, top_p=1.0, seed=SEED)
        order, S, slots = ORDER[:7], 3, 5
        want = [_one_image(eng, inp, b, n * S + j, shape, T, **kw) for n, b in enumerate(order) for j in range(S)]
        ids, lens, steps = eng.generate_stream_sampled(*_args(inp, order), max_length=T, num_return=S, chunk=2, slots=slots, pool_chunks=3, **kw)
        ids, lens = _np(eng, ids), _np(eng, lens)
        assert ids.shape == (7 * S, T) and lens.shape == (7 * S,)
        _check_rows(ids, lens, want, shape)
        varied = sum(1 for n in range(7) if any(not np.array_equal(ids[n * S], ids[n * S + j]) for j in range(1, S)))
        print(f"{varied} of 7 images have samples that differ; {steps} steps for {int(sum(lens - 1))} tokens on {slots} slots")
        assert varied >= 4
        total_tokens = int(sum(int(l) - 1 for l in lens))
        assert steps >= -(-total_tokens // slots)
    finally:
        eng.set_cross_absorb("auto")


@pytest.mark.parametrize("be_name", BACKENDS)
def test_greedy_equivalent_options_give_the_greedy_queue(be_name):
    eng, inp, shape, T, g = _case(be_name)
    q = _args(inp, ORDER)
    geo = dict(max_length=T, chunk=4, slots=3, pool_chunks=2)
    ref_ids, ref_lens, _ = eng.generate_stream(*q, **geo)
    ref_ids, ref_lens = _np(eng, ref_ids), _np(eng, ref_lens)
    for opt in (dict(top_k=1, temperature=0.7), dict(top_k=0, top_p=1e-6)):
        ids, lens, _, ts = eng.generate_stream_sampled(*q, seed=3, return_scores=True, **opt, **geo)
        assert np.array_equal(_np(eng, ids), ref_ids), opt
        assert np.array_equal(_np(eng, lens), ref_lens), opt
        assert np.all(_np(eng, ts) == 0.0), opt


@pytest.mark.parametrize("be_name", BACKENDS)
def test_forced_length_scores_and_small_queues(be_name):
    """EOS suppressed: every column is a draw.  The scores are the batch form's arithmetic on identical logits: exactly equal."""
    eng, inp, shape, _, g = _case(be_name)
    eng.set_cross_absorb(False)
    try:
        T = 12
        kw = dict(temperature=1.5, top_k=0, top_p=1.0, seed=77, min_length=T)
        order = ORDER[:7]
        want = [_one_image(eng, inp, b, n, shape, T, **kw) for n, b in enumerate(order)]
        ids, lens, _, ts = eng.generate_stream_sampled(*_args(inp, order), max_length=T, chunk=4, slots=4, pool_chunks=2, return_scores=True, **kw)
        ids, lens, ts = _np(eng, ids), _np(eng, lens), _np(eng, ts)
        assert np.all(lens == T) and not np.any(ids[:, 1:] == shape.eos_token_id)
        assert np.all(ts < 0)
        for n, (row, _, sc) in enumerate(want):
            assert np.array_equal(ids[n], row), n
            assert np.array_equal(ts[n], sc), (n, ts[n], sc)
        for N, slots in ((1, 4), (2, 8)):
            ids2, lens2, _, ts2 = eng.generate_stream_sampled(*_args(inp, order[:N]), max_length=T, chunk=4, slots=slots, pool_chunks=2,
                                                              return_scores=True, **kw)
            assert np.array_equal(_np(eng, ids2), ids[:N]) and np.all(_np(eng, lens2) == T) and np.array_equal(_np(eng, ts2), ts[:N])
    finally:
        eng.set_cross_absorb("auto")


@pytest.mark.parametrize("be_name", BACKENDS)
def test_graph_key_holds_every_sampling_parameter(be_name):
    """Back-to-back calls on one engine (hip: the captured queue step is replayed or re-captured by its key)."""
    eng, inp, shape, T, g = _case(be_name, "g0_tiny.npz")
    fresh, _, _, _, _ = _case(be_name, "g0_tiny.npz")
    a = _args(inp, np.arange(inp["input_ids"].shape[0]))
    N = a[0].shape[0]
    geo = dict(max_length=T, min_length=T, chunk=2, slots=3, pool_chunks=2)      # no early stop: every column is a draw
    kw = dict(temperature=1.5, top_k=0, top_p=1.0, **geo)

    def run(e=eng, **over):
        r = e.generate_stream_sampled(*a, **dict(kw, **over))
        return (_np(e, r[0]),) + tuple(r[1:])

    g_want = _np(fresh, fresh.generate_stream(*a, **geo)[0])
    b_ids, b_lens, b_sc, _ = fresh.generate_stream_beam(*a, num_beams=3, **geo)
    b_want = (_np(fresh, b_ids), _np(fresh, b_lens), _np(fresh, b_sc))

    a1 = run(seed=101)[0]
    b1 = run(seed=202)[0]
    assert np.array_equal(a1, run(seed=101)[0])
    assert not np.array_equal(a1, b1)
    assert not np.array_equal(a1, run(seed=101, temperature=0.3)[0]), "another temperature, other draws from the same random numbers"
    assert np.array_equal(run(seed=101, top_k=1)[0], g_want)
    assert np.array_equal(run(seed=101, top_p=1e-6)[0], g_want)
    assert np.array_equal(a1, run(seed=101)[0])
    assert np.array_equal(a1, run(seed=101, stream_ids=np.arange(N))[0]), "default stream ids are the sequence indices"
    assert not np.array_equal(a1, run(seed=101, stream_ids=np.arange(N) + 1000)[0])
    assert np.array_equal(a1, run(seed=101)[0])
    # the greedy and the beam queue in between return what a fresh engine returns, and leave nothing behind
    assert np.array_equal(_np(eng, eng.generate_stream(*a, **geo)[0]), g_want)
    assert np.array_equal(a1, run(seed=101)[0])
    ids, lens, sc, _ = eng.generate_stream_beam(*a, num_beams=3, **geo)
    assert np.array_equal(_np(eng, ids), b_want[0]) and np.array_equal(_np(eng, lens), b_want[1]) and np.array_equal(_np(eng, sc), b_want[2])
    assert np.array_equal(a1, run(seed=101)[0])
    # with and without token scores: the same ids
    r = run(seed=101, return_scores=True)
    assert np.array_equal(a1, r[0]) and np.all(_np(eng, r[3]) < 0)
    assert np.array_equal(a1, run(seed=101)[0])
    # num_return 1, 2, 1: sample 0 of image n under num_return = 2 is sequence 2 n
    two = run(seed=101, num_return=2)[0]
    assert two.shape == (2 * N, T)
    assert np.array_equal(two[0::2], run(seed=101, stream_ids=np.arange(N) * 2)[0])
    assert not np.array_equal(two[0::2], two[1::2])
    assert np.array_equal(a1, run(seed=101)[0])


@pytest.mark.parametrize("be_name", BACKENDS)
def test_bad_arguments_name_themselves(be_name):
    eng, inp, shape, T, g = _case(be_name)
    q = _args(inp, ORDER)
    geo = dict(max_length=T, chunk=4, slots=3, pool_chunks=2)
    err = (MgError, ValueError)
    ref_ids, ref_lens, _ = eng.generate_stream(*q, **geo)
    with pytest.raises(err, match="temperature"):
        eng.generate_stream_sampled(*q, temperature=0.0, **geo)
    with pytest.raises(err, match="top_p"):
        eng.generate_stream_sampled(*q, top_p=0.0, **geo)
    with pytest.raises(err, match="top_p"):
        eng.generate_stream_sampled(*q, top_p=1.5, **geo)
    with pytest.raises(err, match="top_k"):
        eng.generate_stream_sampled(*q, top_k=-1, **geo)
    with pytest.raises(err, match="num_return"):
        eng.generate_stream_sampled(*q, num_return=0, **geo)
    with pytest.raises(err, match="stream_ids"):
        eng.generate_stream_sampled(*q, num_return=2, stream_ids=np.arange(len(ORDER)), **geo)
    with pytest.raises(err, match="slots"):
        eng.generate_stream_sampled(*q, max_length=T, chunk=2, slots=9, pool_chunks=2)             # 4 pool entries x 1 sample
    with pytest.raises(err, match="slots"):
        eng.generate_stream_sampled(*q, max_length=T, chunk=2, slots=9, pool_chunks=2, num_return=2)      # 4 entries x 2 samples = 8 rows
    # the library's own checks (the binding refuses these before the call): options straight through the C ABI
    import ctypes as C
    from markushgrapher_amd.engine import MgSampleOpts
    ids, bb, am, pv, N, L = eng._inputs(*q)
    out, ln = eng.mem.empty((N, T), np.int64), eng.mem.empty((N,), np.int32)
    for name, opts in (("temperature", MgSampleOpts(0.0, 0, 1.0, 1, None, 1, None)), ("top_k", MgSampleOpts(1.0, -1, 1.0, 1, None, 1, None)),
                       ("top_p", MgSampleOpts(1.0, 0, 0.0, 1, None, 1, None)), ("top_p", MgSampleOpts(1.0, 0, 1.5, 1, None, 1, None)),
                       ("num_return", MgSampleOpts(1.0, 0, 1.0, 1, None, 0, None))):
        rc = eng.lib.mg_generate_stream_sampled(eng.model, eng.mem.stream(), eng.mem.ptr(eng._sws), eng._sws_bytes, eng.mem.ptr(ids), eng.mem.ptr(bb),
                                                eng.mem.ptr(am), eng.mem.ptr(pv), N, L, 4, 3, 2, T, 0, eng.mem.ptr(out), eng.mem.ptr(ln), None,
                                                C.byref(opts))
        assert rc < 0 and name in eng.lib.mg_last_error().decode() and "mg_generate_stream_sampled" in eng.lib.mg_last_error().decode(), name
    # the engine still runs the greedy-equivalent call
    ids, lens, _ = eng.generate_stream_sampled(*q, top_k=1, seed=3, **geo)
    assert np.array_equal(_np(eng, ids), _np(eng, ref_ids)) and np.array_equal(_np(eng, lens), _np(eng, ref_lens))
