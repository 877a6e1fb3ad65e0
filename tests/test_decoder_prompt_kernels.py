"""The decoder prompt at operator level (include/mgrapher.h mgk_select_prompted, mgk_sample_select_prompted, mgk_beam_init_prompted,
mgk_beam_step_prompted), on scripted logits.

Greedy scan, fused tail and sampled selection run a whole call column by column on the launch's own state (unfinished flags, step
counters).  The model of a forced column is the header's rule: the prompt's token is written, the row stays unfinished even on EOS, its
token score is 0.0, and the step counters see a live row.  Free columns are compared with the UNPROMPTED kernel on the same logits and
flags: ids exactly, token scores bit for bit.  Beam search is compared step by step with the float64 restatement of
tests/prompt_script.py (pinned to stock in tests/test_decoder_prompt_stock.py): sequences and beam indices exactly, scores within the
2e-5 that tests/test_beam_stock.py allows for float32 sums."""
import ctypes as C

import numpy as np
import pytest

from tests import prompt_script
from tests.backends import get_backend
from tests.beam_script import Script, tie_free
from tests.test_beam_kernels import EOS, NAN_PAD, START, Logits, _lib as beam_lib, _read, _write, er_mid
from tests.test_selection_step import (BACKENDS, SENT_ID, SENT_TS, WIN, FusedEnv, Outs, SelDesc, get, lib_of, noise, padded, ptr, ref_step,
                                       same_bits, upload)

MG_E_ARG = -2
V37, MAX_LEN = 37, 8


def prompted_lib(be):
    lib, P, I, F = lib_of(be), C.c_void_p, C.c_int, C.c_float
    lib.mgk_select_prompted.argtypes = [P, P, P, P, I, I, P]
    lib.mgk_sample_select_prompted.argtypes = [P, P, I, I, I, I, I, I, F, I, F, C.c_uint64, P, P, P, I, I, P, P, P, P, P, I, P, P, I, I, P]
    return lib


def desc(o, *, rows, V, max_len, pos, eos, pad, min_len, fused=0, logits=None, ldl=0, pos_dev=None, step_ctr=None, fz=None):
    d = SelDesc()
    d.fused, d.logits, d.rows, d.V, d.ldl, d.eos, d.pad = fused, ptr(logits), rows, V, ldl, eos, pad
    for k in range(3):
        d.eos_more[k] = -1
    d.next_ids, d.out_ids, d.max_len, d.pos, d.pos_dev, d.min_len = o.next.ptr, o.out.ptr, max_len, pos, pos_dev, min_len
    d.unfinished, d.n_unfinished, d.step_ctr = o.unf.ptr, o.n_unf.ptr, step_ctr
    if fz is not None:
        d.ptop, d.stopv, d.ntiles, d.tok_emb, d.h, d.gain = fz["ptop"].ptr, fz["stopv"].ptr, (V + 31) // 32, fz["emb"].ptr, fz["h"].ptr, fz["gain"].ptr
        d.x_pk, d.x2_pk, d.x2_ld, d.x2_col0, d.d, d.eps = fz["x_pk"].ptr, ptr(fz.get("x2")), fz.get("x2_ld", 0), fz.get("x2_col0", 0), fz["d"], fz["eps"]
    d.token_scores, d.ts_ld = ptr(o.ts), max_len - 1
    return d


def make_prompts(lens, V, eos, ld, seed, bad_at=None):
    """[owners][ld] int64: start token 1, then tokens of [8, V); the longest prompt holds a forced EOS; columns past a prompt's length hold an
    id that must never be read (V + 100); bad_at = (owner, column): an id outside [0, V) there"""
    r = np.random.RandomState(seed)
    p = np.full((len(lens), ld), V + 100, np.int64)
    for b, n in enumerate(lens):
        p[b, :n] = [1] + list(r.randint(8, V, n - 1))
        if n >= 3:
            p[b, n - 2] = eos
    if bad_at is not None:
        p[bad_at] = V + 5 if bad_at[1] % 2 else -3
    return p


def step_logits(rows, V, col, eos, seed):
    """noise with a placed winner; EOS wins where (row + col) % 5 == 0; an exact tie (lowest index wins) where (row + col) % 7 == 3"""
    lg = noise(rows, V, seed + 31 * col)
    r = np.random.RandomState(seed + col)
    win = r.randint(8, V - 1, rows)
    lg[np.arange(rows), win] = WIN
    for i in range(rows):
        if (i + col) % 5 == 0:
            lg[i, eos] = WIN + 1
        elif (i + col) % 7 == 3:
            lg[i, win[i] + 1] = WIN                               # tie with the next index: win[i] stays the answer
    return lg


def run_greedy(be, rows, lens, group, fused, dev_pos, bad_at=None, min_len=4):
    """a whole prompted greedy call on the selection kernel, columns 1 .. MAX_LEN - 1 in order, checked at every column"""
    lib = prompted_lib(be)
    V, ldl, eos, pad, max_len = V37, 40, 7, 3, MAX_LEN
    owners = rows // group
    ld = max(lens)
    prompts = make_prompts(lens, V, eos, ld, 5, bad_at)
    P, LEN, BAD = be.buf(prompts), be.buf(np.asarray(lens, np.int32)), be.buf(np.zeros(1, np.int32))
    ctr = be.buf(np.array([rows, -1, 0, 0, 0, 0, 0, 0], np.int32))
    o = Outs(be, rows, max_len, np.ones(rows, np.int32), top2_cols=None)
    upload(o.ts, np.zeros((rows, max_len - 1), np.float32))       # the engine clears the scores of a call; forced columns stay 0
    env = FusedEnv(be, rows, V, 64, True) if fused else None
    unf = np.ones(rows, np.int32)
    want_ids = np.full((rows, max_len), SENT_ID, np.int64)
    want_ts = np.zeros((rows, max_len - 1), np.float32)
    n_bad, done_step = 0, -1
    for col in range(1, max_len):
        lg = step_logits(rows, V, col, eos, 900)
        sup = col < min_len
        emit, _, still, _, sc = ref_step(lg, unf, [eos], pad, sup)
        forced = np.array([col < lens[r // group] for r in range(rows)])
        for r in np.nonzero(forced)[0]:
            t = int(prompts[r // group, col])
            if t < 0 or t >= V:
                t, n_bad = 0, n_bad + 1
            emit[r], still[r] = t, 1
            assert unf[r] == 1                                    # a row in its prompt has never finished
        kw = dict(rows=rows, V=V, max_len=max_len, eos=eos, pad=pad, min_len=min_len, fused=fused,
                  logits=None if fused else be.buf(padded(lg, ldl)), ldl=0 if fused else ldl)
        # the unprompted kernel on the same logits and flags (first: env.fz hands out fresh activation buffers, the prompted launch's are
        # the ones check_next_step reads)
        s = Outs(be, rows, max_len, unf, top2_cols=None)
        sd = desc(s, pos=col, fz=env.fz(lg, [eos]) if fused else None, **kw)
        assert lib.mgk_select_ex(be.stream, C.byref(sd)) == 0
        # the engine's two position forms: the column by value, or 1 + the device step counter (counters[2]; graph replay)
        d = desc(o, pos=1 if dev_pos else col, pos_dev=ctr.ptr + 8 if dev_pos else None, step_ctr=ctr.ptr,
                 fz=env.fz(lg, [eos]) if fused else None, **kw)
        assert lib.mgk_select_prompted(be.stream, C.byref(d), P.ptr, LEN.ptr, ld, group, BAD.ptr) == 0
        out, ts, nxt = get(o.out), get(o.ts), get(o.next)
        assert np.array_equal(nxt, emit) and np.array_equal(out[:, col], emit), (col, nxt, emit)
        assert np.array_equal(get(o.unf), still), col
        free = ~forced
        assert np.array_equal(nxt[free], get(s.next)[free])
        same_bits(ts[free, col - 1], get(s.ts)[free, col - 1], "token scores of free rows against the unprompted kernel, column %d" % col)
        assert np.all(ts[forced, col - 1] == 0)
        np.testing.assert_allclose(ts[free, col - 1], sc[free], rtol=1e-5, atol=1e-6)
        if fused:
            env.check_next_step(emit)                             # h / x_pk / x2 = embed_norm_rows of the EMITTED (forced) token
        # counters: the unfinished count published, the first all-finished step recorded once, the step advanced, nothing left over
        c = get(ctr)
        if still.sum() == 0 and done_step < 0:
            done_step = col - 1
        assert (int(c[0]), int(c[1]), int(c[2]), int(c[6]), int(get(o.n_unf)[0])) == (int(still.sum()), done_step, col, 0, 0), (col, c)
        want_ids[:, col] = emit
        want_ts[:, col - 1] = ts[:, col - 1]
        unf = still
    assert np.array_equal(get(o.out)[:, 1:], want_ids[:, 1:]) and np.all(get(o.out)[:, 0] == SENT_ID)
    same_bits(get(o.ts), want_ts, "token scores of the run")
    assert int(get(BAD)[0]) == n_bad == (0 if bad_at is None else 1)
    return want_ids


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("dev_pos", [False, True], ids=["pos", "pos_dev"])
@pytest.mark.parametrize("fused", [0, 1], ids=["scan", "fused"])
def test_greedy_three_rows(be_name, fused, dev_pos):
    """3 rows, V = 37 (no multiple of 4), max_len 8, prompt lengths [1, 3, 5]: forced columns hold the prompt, free columns the lowest index
    of the maximum; the forced EOS of row 2 (column 3) leaves it unfinished; scores and counters as the module's header says."""
    be = get_backend(be_name)
    ids = run_greedy(be, 3, [1, 3, 5], 1, fused, dev_pos)
    assert ids[2, 3] == 7 and ids[1, 1] == 7                     # the forced EOS tokens were written ...
    assert (ids[2, 5:] != 3).any()                               # ... and row 2 went on decoding after its prompt (pad = 3 only after a free EOS)


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("fused", [0, 1], ids=["scan", "fused"])
def test_greedy_bad_prompt_id(be_name, fused):
    """a prompt id outside [0, V) is replaced by id 0 and counted; it never indexes the embedding table (the fused tail embeds row 0)"""
    be = get_backend(be_name)
    for bad_at in ((2, 3), (1, 2)):                              # V + 5 and -3
        ids = run_greedy(be, 3, [1, 3, 5], 1, fused, False, bad_at=bad_at)
        assert ids[bad_at] == 0


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("fused", [0, 1], ids=["scan", "fused"])
def test_greedy_256_rows(be_name, fused):
    """256 rows, prompt lengths cycling 1 .. 7 (the row * ld + col indexing), the device-counter form"""
    run_greedy(get_backend(be_name), 256, [1 + r % 7 for r in range(256)], 1, fused, True)


@pytest.mark.parametrize("be_name", BACKENDS)
def test_greedy_rows_share_their_owners_prompt(be_name):
    """group = 2: rows 2b and 2b + 1 take prompt b (the samples of an image)"""
    run_greedy(get_backend(be_name), 6, [1, 3, 5], 2, 0, False)


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("dev_pos", [False, True], ids=["pos", "pos_dev"])
@pytest.mark.parametrize("rows,group", [(3, 1), (6, 2)])
def test_sampled_selection(be_name, rows, group, dev_pos):
    """sample_select under a prompt: forced rows write the prompt, score 0 and stay live; in each free column token and score equal the
    unprompted kernel's at the same (seed, stream id, column) - the forced columns consumed no draw.  pos_dev: the column is 1 + the
    step counter that the launch itself advances (a forced row's threads must all have read it before its bookkeeping runs)."""
    be = get_backend(be_name)
    lib = prompted_lib(be)
    V, ldl, eos, pad, max_len, min_len = V37, 40, 7, 3, MAX_LEN, 4
    lens = [1, 3, 5]
    ld, seed, T, top_k, top_p = 5, 0x1234567, 0.8, 12, 0.9
    prompts = make_prompts(lens, V, eos, ld, 6)
    P, LEN, BAD = be.buf(prompts), be.buf(np.asarray(lens, np.int32)), be.buf(np.zeros(1, np.int32))
    sids = be.buf((1000 + 17 * np.arange(rows)).astype(np.uint64).view(np.int64))
    ctr = be.buf(np.array([rows, -1, 0, 0, 0, 0, 0, 0], np.int32))
    o = Outs(be, rows, max_len, np.ones(rows, np.int32), top2_cols=None)
    upload(o.ts, np.zeros((rows, max_len - 1), np.float32))
    unf = np.ones(rows, np.int32)
    saw_free_after_forced = False
    for col in range(1, max_len):
        lg = be.buf(padded(step_logits(rows, V, col, eos, 70), ldl))
        assert lib.mgk_sample_select_prompted(be.stream, lg.ptr, rows, V, ldl, eos, pad, min_len, T, top_k, top_p, seed, sids.ptr, o.next.ptr,
                                              o.out.ptr, max_len, 1 if dev_pos else col, ctr.ptr + 8 if dev_pos else None, o.unf.ptr,
                                              o.n_unf.ptr, ctr.ptr, o.ts.ptr, max_len - 1, P.ptr,
                                              LEN.ptr, ld, group, BAD.ptr) == 0
        s = Outs(be, rows, max_len, unf, top2_cols=None)
        assert lib.mgk_sample_select(be.stream, lg.ptr, rows, V, ldl, eos, pad, min_len, T, top_k, top_p, seed, sids.ptr, s.next.ptr, s.out.ptr,
                                     max_len, col, s.unf.ptr, s.n_unf.ptr, s.ts.ptr, max_len - 1) == 0
        forced = np.array([col < lens[r // group] for r in range(rows)])
        nxt, ts, still = get(o.next), get(o.ts), get(o.unf)
        want = np.where(forced, prompts[np.arange(rows) // group, min(col, ld - 1)], get(s.next))
        assert np.array_equal(nxt, want) and np.array_equal(get(o.out)[:, col], want), col
        assert np.all(ts[forced, col - 1] == 0)
        same_bits(ts[~forced, col - 1], get(s.ts)[~forced, col - 1], "scores of free rows, column %d" % col)
        assert np.array_equal(still, np.where(forced, 1, get(s.unf))), col
        if col < min_len:
            assert not (nxt[~forced] == eos).any()
        c = get(ctr)
        assert (int(c[0]), int(c[2]), int(c[6]), int(get(o.n_unf)[0])) == (int(still.sum()), col, 0, 0)
        saw_free_after_forced = saw_free_after_forced or bool((~forced & (unf == 1))[group:].any())
        unf = still
    assert saw_free_after_forced and int(get(BAD)[0]) == 0


# ---- beam search ------------------------------------------------------------------------------------------------------------------
def run_beam(be, script, B, K, max_length, prompts, ref, dev_pos=False, min_length=0, length_penalty=1.0, early_stopping=False,
             num_return=1, pad=0, bad=None):
    """the batch form as mg_generate_prompted enqueues it, checked against `ref` (prompt_script.reference) at every step"""
    lib = beam_lib(be)
    V, R = script.V, B * K
    ldl, T_cap = V + 14, max_length - 1
    lens = [len(p) for p in prompts]
    ld = max(lens) + 1
    pid = np.full((B, ld), V + 100, np.int64)                     # (columns past a prompt's length are never read)
    for b, p in enumerate(prompts):
        pid[b, :len(p)] = p
    if bad is not None:
        pid[bad] = V + 7
    PID, LEN, BAD = be.buf(pid), be.buf(np.asarray(lens, np.int32)), be.buf(np.zeros(1, np.int32))
    state = be.zeros(lib.mgk_beam_state_bytes(B, K, max_length), np.uint8)
    nid, bidx, ctr = be.zeros(R, np.int64), be.zeros(R, np.int32), be.zeros(8, np.int32)
    anc = be.zeros((T_cap, R), np.int32)
    div = be.buf(np.array([lib.mgk_beam_length_divisor(c, length_penalty) for c in range(max_length + 1)], np.float32))
    tdev = be.zeros(1, np.int32)
    lg = Logits(be, R, V, ldl, NAN_PAD)
    s = be.stream
    assert lib.mgk_beam_init_prompted(s, be.p(state), B, K, max_length, pad, EOS, START, be.p(nid), be.p(anc), T_cap, be.p(ctr), be.p(PID),
                                      be.p(LEN), ld, V, be.p(BAD)) == 0
    first = _read(be, nid)
    assert np.array_equal(first, np.repeat([0 if bad == (b, 0) else prompts[b][0] for b in range(B)], K))
    prefixes = [[int(first[r])] for r in range(R)]
    anc_ref = np.tile(np.arange(R, dtype=np.int32), (T_cap, 1))
    n_steps = 0
    for t in range(max_length - 1):
        lg.set({r: script.logits(r // K, prefixes[r]) for r in range(R)})
        if dev_pos:
            _write(be, tdev, np.array([t], np.int32))
        assert lib.mgk_beam_step_prompted(s, be.p(state), be.p(lg.dev), ldl, V, B, K, max_length, t + 1, be.p(tdev) if dev_pos else None,
                                          be.p(div), EOS, min_length, C.c_float(length_penalty), int(early_stopping), be.p(nid), be.p(bidx),
                                          be.p(ctr), be.p(PID), be.p(LEN), ld) == 0
        assert lib.mgk_beam_reorder_anc(s, be.p(anc), be.p(bidx), R, max_length - 1 if dev_pos else t + 1, be.p(tdev) if dev_pos else None,
                                        be.p(ctr), None, None) == 0
        n, bi, cont = _read(be, nid), _read(be, bidx), bool(_read(be, ctr)[0])
        n_steps += 1
        if ref is not None:
            rs = ref["steps"][t]
            assert np.array_equal(n, rs["next_ids"]), ("next_ids", t, n, rs["next_ids"])
            assert np.array_equal(bi, rs["beam_idx"]), ("beam_idx", t, bi, rs["beam_idx"])
            assert cont == rs["cont"], ("continue flag", t)
        if cont:
            anc_ref[:t + 1] = anc_ref[:t + 1][:, bi]
        assert np.array_equal(_read(be, anc), anc_ref), ("ancestor table", t)
        prefixes = [prefixes[bi[r]] + [int(n[r])] for r in range(R)]
        if not cont:
            break
    nr = num_return
    out_ids, out_cols, out_sc = be.zeros((B * nr, max_length), np.int64), be.zeros(1, np.int32), be.zeros(B * nr, np.float32)
    obi, ots = be.zeros((B * nr, max_length - 1), np.int32), be.zeros((B * nr, max_length - 1), np.float32)
    assert lib.mgk_beam_finalize(s, be.p(state), B, K, max_length, be.p(out_ids), be.p(out_cols), be.p(out_sc), nr, be.p(obi), be.p(ots)) == 0
    return dict(n_steps=n_steps, out_ids=_read(be, out_ids), cols=int(_read(be, out_cols)[0]), scores=_read(be, out_sc),
                beam_indices=_read(be, obi), token_scores=_read(be, ots), bad=int(_read(be, BAD)[0]))


def check_beam(out, ref, lens, K, nr):
    seq = ref["sequences"]
    n = seq.shape[1] - 1
    assert out["n_steps"] == len(ref["steps"]) and out["cols"] == 1 + n
    assert np.array_equal(out["out_ids"][:, :1 + n], seq)
    assert np.array_equal(out["beam_indices"][:, :n], ref["beam_indices"])
    assert (out["beam_indices"][:, n:] == -1).all() and (out["token_scores"][:, n:] == 0).all()
    for b, P in enumerate(lens):                                  # forced columns: the image's beam-0 flat row, score exactly 0
        rows = slice(b * nr, (b + 1) * nr)
        assert (out["beam_indices"][rows, :P - 1] == b * K).all() and (out["token_scores"][rows, :P - 1] == 0).all()
    np.testing.assert_allclose(out["token_scores"][:, :n], ref["token_scores"], rtol=0, atol=2e-5)
    np.testing.assert_allclose(out["scores"], ref["scores"], rtol=0, atol=2e-5)


def beam_prompts(lens, V, seed=0):
    r = np.random.RandomState(50 + seed)
    out = [[START] + [int(t) for t in r.choice(np.arange(10, V), n - 1, replace=False)] for n in lens]
    b = int(np.argmax(lens))
    if lens[b] >= 3:
        out[b][lens[b] - 2] = EOS                                 # a forced EOS finishes nothing
    return out


BEAM = [
    # (B, K, V, max_length, prompt lengths, options)
    (2, 3, 50, 12, [1, 4], dict()),
    (2, 3, 50, 12, [1, 1], dict()),                                                             # [start] alone
    (2, 5, 50, 12, [1, 4], dict(length_penalty=0.7, num_return=5)),
    (2, 5, 50, 12, [5, 2], dict(length_penalty=0.0, early_stopping=True, num_return=5)),
    (3, 5, 60, 14, [3, 1, 6], dict(min_length=6, num_return=5, early_stopping=False, pad=3)),   # min_length in the middle
    (2, 5, 50, 12, [4, 4], dict(early_stopping=True, min_length=5, length_penalty=0.7)),
    (1, 2, 50, 6, [5], dict(num_return=2)),                                                     # one free column: every candidate hits
]


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("case", BEAM, ids=lambda c: "B%dK%dP%s-%s" % (c[0], c[1], "_".join(map(str, c[4])), "-".join("%s%s" % (k[:3], v) for k, v in c[5].items())))
def test_beam_against_restatement(be_name, case):
    B, K, V, ml, lens, o = case
    be = get_backend(be_name)
    prompts = beam_prompts(lens, V)
    script, ref = tie_free(lambda seed: Script(V, EOS, seed=seed, eos_rank=er_mid, n_hot=20),
                           lambda s: prompt_script.reference(s, B, K, ml, prompts, **o))
    nr = o.get("num_return", 1)
    a = run_beam(be, script, B, K, ml, prompts, ref, **o)
    check_beam(a, ref, lens, K, nr)
    b = run_beam(be, script, B, K, ml, prompts, ref, dev_pos=True, **o)      # the device-counter form: the same bits
    for k in ("out_ids", "scores", "beam_indices", "token_scores"):
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    assert a["cols"] == b["cols"] and a["bad"] == b["bad"] == 0


@pytest.mark.parametrize("be_name", BACKENDS)
def test_beam_start_prompt_is_the_unprompted_step(be_name):
    """a prompt of [start] alone: the state after every step equals the unprompted entries' bit for bit"""
    from tests.test_beam_kernels import run_batch
    be = get_backend(be_name)
    B, K, V, ml = 2, 3, 50, 12
    o = dict(length_penalty=0.7, num_return=3, min_length=3)
    script = Script(V, EOS, seed=3, kind="grid", eos_rank=er_mid, n_hot=20)
    u = run_batch(be, script, B, K, ml, ldl=V + 14, **o)
    p = run_beam(be, script, B, K, ml, [[START]] * B, None, **o)
    for k in ("out_ids", "scores", "beam_indices", "token_scores"):
        assert np.array_equal(u[k].view(np.uint8), p[k].view(np.uint8)), k
    assert u["cols"] == p["cols"] and len(u["steps"]) == p["n_steps"]


@pytest.mark.parametrize("be_name", BACKENDS)
def test_beam_bad_prompt_id(be_name):
    """an id outside [0, V) in a prompt: replaced by id 0 in every beam, counted once per (image, column)"""
    be = get_backend(be_name)
    B, K, V, ml, lens = 2, 3, 50, 8, [1, 4]
    prompts = beam_prompts(lens, V)
    fixed = [list(p) for p in prompts]
    fixed[1][2] = 0
    script = Script(V, EOS, seed=1, kind="grid", eos_rank=er_mid, n_hot=20)
    ref = prompt_script.reference(script, B, K, ml, fixed)
    out = run_beam(be, script, B, K, ml, prompts, ref, bad=(1, 2))
    assert out["bad"] == 1
    assert np.array_equal(out["out_ids"][:, :out["cols"]], ref["sequences"])


@pytest.mark.parametrize("be_name", BACKENDS)
def test_prompted_entries_validate(be_name):
    be = get_backend(be_name)
    lib = prompted_lib(be)
    blib = beam_lib(be)
    o = Outs(be, 2, 4, np.ones(2, np.int32), top2_cols=None)
    lg = be.buf(np.zeros((2, 40), np.float32))
    d = desc(o, rows=2, V=37, max_len=4, pos=1, eos=7, pad=0, min_len=0, logits=lg, ldl=40)
    P, LEN = be.buf(np.ones((2, 2), np.int64)), be.buf(np.ones(2, np.int32))
    assert lib.mgk_select_prompted(be.stream, C.byref(d), None, LEN.ptr, 2, 1, None) == MG_E_ARG
    assert lib.mgk_select_prompted(be.stream, C.byref(d), P.ptr, None, 2, 1, None) == MG_E_ARG
    assert lib.mgk_select_prompted(be.stream, C.byref(d), P.ptr, LEN.ptr, 0, 1, None) == MG_E_ARG
    tab = be.zeros(16, np.int32)
    d.slots.pos, d.slots.img, d.slots.ctr, d.slots.out_len = tab.ptr, tab.ptr, tab.ptr, tab.ptr
    assert lib.mgk_select_prompted(be.stream, C.byref(d), P.ptr, LEN.ptr, 2, 1, None) == MG_E_ARG      # a slot table with a prompt
    state = be.zeros(blib.mgk_beam_state_bytes(1, 2, 4), np.uint8)
    nid, bidx, ctr, anc = be.zeros(2, np.int64), be.zeros(2, np.int32), be.zeros(8, np.int32), be.zeros((3, 2), np.int32)
    assert blib.mgk_beam_init_prompted(be.stream, be.p(state), 1, 2, 4, 0, 7, 1, be.p(nid), be.p(anc), 3, be.p(ctr), None, be.p(LEN), 2, 37,
                                       None) == MG_E_ARG
    assert blib.mgk_beam_step_prompted(be.stream, be.p(state), be.p(lg), 40, 37, 1, 2, 4, 1, None, None, 7, 0, C.c_float(1.0), 0, be.p(nid),
                                       be.p(bidx), be.p(ctr), be.p(P), be.p(LEN), 2) == MG_E_ARG       # no divisor table
