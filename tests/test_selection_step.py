"""The selection step that ends every decode step, at operator level, in every form the decode loops launch it in:

  A  greedy_select_kernel, batch form (mgk_select_ex, fused = 0): ocr.hip's batch loop and its column-0 selection; engine.hip decode_step's
     K == 1 branch when the tail is not fused (pos_dev / top2 [max_len][rows][2] / step_ctr under graph replay; eos_more = the OCR stop list)
  B  greedy_select_fused_kernel (fused = 1): engine.hip decode_step's K == 1 branch on the lm_head partials (TopOut), which also produces the
     next step's h / x_pk / x2 window (embed_norm_rows' work)
  C  the queue form of both selection kernels (the `stream` branch of greedy_select_kernel: engine.hip mg_generate_stream and ocr.hip's queue;
     sample_select_kernel<.., QUEUE = true>, all three instantiations: mg_generate_stream_sampled), one launch on a slot table
  D  slot_refill_kernel against a Python model of the slot table, single launches and a scripted queue run (select + refill per step)
  E  the argument checks of the three entries

References are plain numpy in float64 from stock's semantics (argmax with lowest-index tie-break, finished rows emit pad, MinLength
suppression, log-softmax over the processed logits); the slot machine's reference is SlotModel below, written from the comments of SlotTable /
slot_refill in csrc/mg_kernels.h and the counters layout in engine.hip.

Inputs are built so that the float64 reference decides every row: noise in [-2, 2], a placed winner at 5.0 or more (margin >= 3), ties are
exactly equal floats placed on purpose.  Ids, flags, counters, top2, h, the x2 window and every "same bits" comparison are exact.

Token scores: rtol 1e-5, atol 1e-6 against float64 (the bound of tests/test_scores.py for these kernels).  It holds at the largest rows used
here: the full-row scan sums exp(x - max) over ceil(V / 4096) * 4 <= 52 terms per thread, then a 6-level wave tree and 15 serial adds: about 73
roundings of 2^-24 in the worst case plus expf's 1 ulp and logf's 1 ulp, i.e. a relative error of the sum below 75 * 6e-8 = 4.5e-6, which is
the ABSOLUTE error of its logarithm; the scores here are about -6.4 (sum ~ 600 at V = 49280), so the bound is 6.4e-5: 14 times that worst
case.  The fused tail merges at most 5 (max, sum) pairs per thread, 6 + 3 more in the trees: fewer roundings still."""
import ctypes as C

import numpy as np
import pytest

from tests import pkutil as pk
from tests.backends import get_backend
from tests.test_ocr_kernels import rms_bound

BACKENDS = [pytest.param("emu"), pytest.param("hip", marks=pytest.mark.gpu)]
MG_E_SHAPE, MG_E_ARG, MG_E_UNSUPPORTED = -1, -2, -5
NEG = np.float32(-3.0e38)           # the kernels' "nothing here"
PADV = np.float32(1.0e30)           # padding columns [V, ldl): larger than every logit, must never decide
SENT_ID, SENT_TS, SENT32 = -7, np.float32(9.0), np.float32(-12345.678)
SENT16, NAN16 = 0xBEEF, 0x7FC1
WIN = np.float32(5.0)
TS_TOL = dict(rtol=1e-5, atol=1e-6)
GS_THREADS, FUSED_THREADS = 1024, 256


class SlotTab(C.Structure):
    _fields_ = [("pos", C.c_void_p), ("img", C.c_void_p), ("pool", C.c_void_p), ("ctr", C.c_void_p), ("out_len", C.c_void_p),
                ("pool_cap", C.c_int), ("start_id", C.c_int), ("first_tok", C.c_void_p), ("n_stop", C.c_int), ("stop", C.c_int * 4),
                ("max_len", C.c_int), ("nsamp", C.c_int)]


class SelDesc(C.Structure):
    _fields_ = [("fused", C.c_int), ("logits", C.c_void_p), ("rows", C.c_int), ("V", C.c_int), ("ldl", C.c_int), ("eos", C.c_int),
                ("pad", C.c_int), ("suppress_eos", C.c_int), ("n_eos_more", C.c_int), ("eos_more", C.c_int * 3), ("next_ids", C.c_void_p),
                ("out_ids", C.c_void_p), ("max_len", C.c_int), ("pos", C.c_int), ("pos_dev", C.c_void_p), ("min_len", C.c_int),
                ("unfinished", C.c_void_p), ("n_unfinished", C.c_void_p), ("top2", C.c_void_p), ("step_ctr", C.c_void_p), ("slots", SlotTab),
                ("ptop", C.c_void_p), ("stopv", C.c_void_p), ("ntiles", C.c_int), ("tok_emb", C.c_void_p), ("h", C.c_void_p),
                ("gain", C.c_void_p), ("x_pk", C.c_void_p), ("x2_pk", C.c_void_p), ("x2_ld", C.c_int), ("x2_col0", C.c_int), ("d", C.c_int),
                ("eps", C.c_float), ("token_scores", C.c_void_p), ("ts_ld", C.c_int)]


def lib_of(be):
    lib, V, I, F = be.lib, C.c_void_p, C.c_int, C.c_float
    lib.mgk_select_ex.argtypes = [V, V]
    sample = [V, V, I, I, I, I, I, I, F, I, F, C.c_uint64, V, V, V, I, I, V, V, V, I]
    lib.mgk_sample_select.argtypes = sample
    lib.mgk_sample_select_queue.argtypes = sample + [V]
    lib.mgk_slot_refill.argtypes = [V, V, V, V, I]
    lib.mgk_embed_norm_rows.argtypes = [V] * 7 + [I] * 5 + [V, F]
    lib.mgk_lm_head_step.argtypes = [V] * 4 + [I] * 4 + [V, I, F, F] + [V] * 3 + [I, I]
    return lib


def ptr(b):
    return b.ptr if b is not None else None


def upload(b, arr):
    """overwrite a backend buffer in place (the test's side of a counter the host raises, or of a logits buffer refilled every step)"""
    arr = np.ascontiguousarray(arr, dtype=b.dtype).reshape(b.shape)
    if b.be.name == "emu":
        b.a[...] = arr
    else:
        import torch
        b.be.sync()
        b.a.copy_(torch.from_numpy(arr.view(np.int16) if arr.dtype == np.uint16 else arr))


def get(b):
    return np.array(b.numpy(), copy=True)


def bits(a):
    a = np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_bits(a, b, what):
    assert a.shape == b.shape, what
    assert np.array_equal(bits(a), bits(b)), "%s: %d of %d elements differ" % (what, int((bits(a) != bits(b)).sum()), a.size)


def noise(rows, V, seed):
    return np.random.RandomState(seed).uniform(-2.0, 2.0, (rows, V)).astype(np.float32)


def padded(lg, ldl, fill=PADV):
    out = np.full((lg.shape[0], ldl), fill, np.float32)
    out[:, :lg.shape[1]] = lg
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# the float64 reference of one selection step (batch form)
# ---------------------------------------------------------------------------------------------------------------------------------------
def ref_step(lg, unf, stops, pad, suppressed):
    """lg [rows][V] float32.  Returns emitted ids, the row's arg-max, unfinished after the step, top-2 of the processed row (float32 values),
    token score (0 for a finished row) - all by the rules, in float64."""
    x = lg.astype(np.float64)
    if suppressed:
        x[:, list(stops)] = -np.inf
    tok = np.argmax(x, axis=1)                                    # numpy: the first (lowest) index of the maximum
    srt = np.sort(x, axis=1)
    top2 = np.maximum(srt[:, -2:][:, ::-1], np.float64(NEG)).astype(np.float32)
    mx = x.max(1, keepdims=True)
    lsm = x[np.arange(len(x)), tok] - mx[:, 0] - np.log(np.exp(x - mx).sum(1))
    unf = np.asarray(unf).astype(bool)
    emit = np.where(unf, tok, pad).astype(np.int64)
    still = (unf & ~np.isin(emit, list(stops))).astype(np.int32)
    return emit, tok, still, top2, np.where(unf, lsm, 0.0)


class Outs:
    """output buffers of a selection launch, every one pre-filled with a sentinel"""

    def __init__(self, be, rows, max_len, unf, n_unf=0, top2_cols=None, scores=True, nseq=None):
        nseq = rows if nseq is None else nseq
        self.next = be.buf(np.full(rows, SENT_ID, np.int64))
        self.out = be.buf(np.full((nseq, max_len), SENT_ID, np.int64))
        self.unf = be.buf(np.asarray(unf, np.int32))
        self.n_unf = be.buf(np.array([n_unf], np.int32))
        self.ts = be.buf(np.full((nseq, max(max_len - 1, 1)), SENT_TS, np.float32)) if scores else None
        self.top2 = None
        if top2_cols is not None:
            self.top2 = be.buf(np.full((top2_cols, rows, 2) if top2_cols else (rows, 2), SENT32, np.float32))


def select(be, o, *, rows, V, max_len, pos, eos, fused=0, logits=None, ldl=0, pad=0, more=(), n_more=None, pos_dev=None, min_len=0,
           step_ctr=None, slots=None, fz=None, expect=0):
    d = SelDesc()
    d.fused, d.logits, d.rows, d.V, d.ldl, d.eos, d.pad = fused, ptr(logits), rows, V, ldl, eos, pad
    d.n_eos_more = len(more) if n_more is None else n_more
    for k in range(3):
        d.eos_more[k] = more[k] if k < len(more) else -1
    d.next_ids, d.out_ids, d.max_len, d.pos, d.pos_dev, d.min_len = o.next.ptr, o.out.ptr, max_len, pos, ptr(pos_dev), min_len
    d.unfinished, d.n_unfinished, d.top2, d.step_ctr = o.unf.ptr, o.n_unf.ptr, ptr(o.top2), ptr(step_ctr)
    if slots is not None:
        d.slots = slots
    if fz is not None:
        d.ptop, d.stopv, d.ntiles, d.tok_emb, d.h, d.gain = fz["ptop"].ptr, fz["stopv"].ptr, (V + 31) // 32, fz["emb"].ptr, fz["h"].ptr, fz["gain"].ptr
        d.x_pk, d.x2_pk, d.x2_ld, d.x2_col0, d.d, d.eps = fz["x_pk"].ptr, ptr(fz.get("x2")), fz.get("x2_ld", 0), fz.get("x2_col0", 0), fz["d"], fz["eps"]
    d.token_scores, d.ts_ld = ptr(o.ts), max(max_len - 1, 1)
    rc = lib_of(be).mgk_select_ex(be.stream, C.byref(d))
    assert rc == expect, rc
    return d


# =======================================================================================================================================
# A. full-row greedy scan, batch form
# =======================================================================================================================================
def scan_rows(V):
    """(winner indices, tie pairs) for a row of V logits under the scan's cut: float4 c belongs to thread c % 1024, load (c / 1024) % 4 of
    batch c / 4096; wave = thread / 64."""
    nq = (V + 3) // 4
    win = [0, V - 1]
    if V % 4:
        win.append(V - 1 - (V - 1) % 4)                           # first element of the partly padded float4, V - 1 is its last real one
    for p in range((nq + 4095) // 4096):                          # one index in each batch a thread visits
        win.append(min(4 * min(p * 4096 + 37, nq - 1) + 2, V - 1))
    if nq > 1000:
        win.append(4 * 1000 + 1)                                  # thread 1000: the last wave
    ties = [(4 * 5 + 1, 4 * 5 + 3), (4 * 5, 4 * 9)]               # inside one float4; two threads of a wave
    if nq > 70:
        ties.append((4 * 5 + 1, 4 * 70 + 1))                      # two waves
    if nq > 1024 + 5:
        ties.append((4 * 5 + 2, 4 * (1024 + 5)))                  # two loads of one batch of thread 5
    if nq > 4096:
        ties.append((4 * 0 + 3, 4 * 4096 + 1))                    # two batches of thread 0: the lower index is met FIRST (a thread's own
        #                                                           visits ascend); then the lower index in a LATER wave's first batch against
        #                                                           the higher one in wave 0's second batch: the merge of the waves meets it LAST
        ties.append((4 * 900 + 2, 4 * 4096 + 2))
    return sorted(set(win)), ties


def scan_case(V, seed):
    win, ties = scan_rows(V)
    rows = len(win) + len(ties) + 1
    lg = noise(rows, V, seed)
    for r, i in enumerate(win):
        lg[r, i] = WIN
    for k, (a, b) in enumerate(ties):
        lg[len(win) + k, [a, b]] = WIN
    expect = win + [a for a, _ in ties] + [int(np.argmax(lg[-1]))]      # the last row: plain noise (the reference decides it all the same)
    return lg, np.array(expect)


SCAN_SHAPES = [(320, 320), (1000, 1024), (16384, 16384), (16388, 16416), (33201, 33216), (49280, 49280)]


def scan_params():
    out = []
    for V, ldl in SCAN_SHAPES:
        for be in BACKENDS:                                        # (the emulator runs the two largest rows in well under a second each)
            out.append(pytest.param(be.values[0], V, ldl, marks=be.marks, id="%s-V%d-ld%d" % (be.values[0], V, ldl)))
    return out


@pytest.mark.parametrize("be_name,V,ldl", scan_params())
def test_greedy_scan_winner_positions_and_ties(be_name, V, ldl):
    """Winner at index 0, V - 1, inside the partly padded float4, in every batch of a thread, in the last wave; exact ties inside a float4,
    between threads, waves, loads and batches (lowest index wins, b2 == b1); padding columns at +1e30.  Launches of 5 rows (one of them
    finished: pad, flag stays 0, score 0, top2 = the row's own top-2 as for a live row) and of 1 row; n_unfinished accumulates on the value the
    caller left."""
    be = get_backend(be_name)
    lg, expect = scan_case(V, 100 + V % 97)
    eos, pad, max_len, pos = 7, 3, 6, 4
    assert not np.isin(expect, [eos]).any()
    L = padded(lg, ldl)
    for r0 in range(0, len(lg), 5):
        sel = np.arange(r0, r0 + 5) % len(lg)
        unf = np.ones(5, np.int32)
        unf[(r0 // 5) % 5] = 0
        emit, tok, still, top2, sc = ref_step(lg[sel], unf, [eos], pad, False)
        assert np.array_equal(tok, expect[sel])
        o = Outs(be, 5, max_len, unf, n_unf=11, top2_cols=0)
        select(be, o, rows=5, V=V, ldl=ldl, logits=be.buf(L[sel]), max_len=max_len, pos=pos, eos=eos, pad=pad)
        out, ts = get(o.out), get(o.ts)
        assert np.array_equal(get(o.next), emit) and np.array_equal(out[:, pos], emit), (get(o.next), emit)
        assert np.all(np.delete(out, pos, 1) == SENT_ID) and np.all(np.delete(ts, pos - 1, 1) == SENT_TS)
        assert np.array_equal(get(o.unf), still) and int(get(o.n_unf)[0]) == 11 + int(still.sum())
        same_bits(get(o.top2), top2, "top2")
        print("V=%d rows %d.. token score max abs err %.3g" % (V, r0, np.abs(ts[:, pos - 1] - sc).max()))
        np.testing.assert_allclose(ts[:, pos - 1], sc, **TS_TOL)
        assert np.all(ts[unf == 0, pos - 1] == 0)
    for r in (0, 1, len(lg) - 2):                                 # one row per launch
        emit, _, still, top2, sc = ref_step(lg[r:r + 1], [1], [eos], pad, False)
        o = Outs(be, 1, max_len, [1], top2_cols=0)
        select(be, o, rows=1, V=V, ldl=ldl, logits=be.buf(L[r:r + 1]), max_len=max_len, pos=pos, eos=eos, pad=pad)
        assert int(get(o.next)[0]) == expect[r] == int(get(o.out)[0, pos]) and int(get(o.n_unf)[0]) == 1
        same_bits(get(o.top2), top2, "top2")
        np.testing.assert_allclose(get(o.ts)[:, pos - 1], sc, **TS_TOL)


@pytest.mark.parametrize("be_name", BACKENDS)
def test_greedy_scan_256_rows(be_name):
    """256 rows at V = 1000, ldl = 1024: every row its own winner (the scenarios of the 5-row test, then random places), every 7th row finished."""
    be = get_backend(be_name)
    V, ldl, eos, pad, max_len, pos = 1000, 1024, 7, 3, 6, 1
    base, exp0 = scan_case(V, 5)
    lg = noise(256, V, 6)
    lg[:len(base)] = base
    where = np.random.RandomState(8).randint(8, V, 256)
    for r in range(len(base), 256):
        lg[r, where[r]] = WIN
    unf = (np.arange(256) % 7 != 3).astype(np.int32)
    emit, tok, still, top2, sc = ref_step(lg, unf, [eos], pad, False)
    assert np.array_equal(tok[:len(base)], exp0) and np.array_equal(tok[len(base):], where[len(base):])
    o = Outs(be, 256, max_len, unf, top2_cols=0)
    select(be, o, rows=256, V=V, ldl=ldl, logits=be.buf(padded(lg, ldl)), max_len=max_len, pos=pos, eos=eos, pad=pad)
    assert np.array_equal(get(o.next), emit) and np.array_equal(get(o.out)[:, pos], emit)
    assert np.array_equal(get(o.unf), still) and int(get(o.n_unf)[0]) == int(still.sum())
    same_bits(get(o.top2), top2, "top2")
    np.testing.assert_allclose(get(o.ts)[:, pos - 1], sc, **TS_TOL)


def stop_rows(V, stops, spare):
    """rows of the stop-list cases for the LAST id of `stops`: it wins; it ties with a lower-index and with a higher-index ordinary token; the
    row is already finished; another stop id is second best; `spare` (an eos_more entry past n_eos_more: no stop token) wins."""
    s = stops[-1]
    lg = noise(7, V, 40 + len(stops))
    lg[0, s] = WIN
    lg[1, [s - 9, s]] = WIN                                       # ordinary token below the stop id: it wins, the row goes on
    lg[2, [s, s + 11]] = WIN                                      # stop id below: the row ends
    lg[3, s] = WIN
    lg[4, s], lg[4, stops[0]] = WIN, WIN - 1                      # suppressed together: the best ordinary token wins
    lg[5, spare] = WIN
    lg[6, 500] = WIN
    return lg, np.array([1, 1, 1, 0, 1, 1, 1], np.int32)


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("n_more", [0, 1, 3])
def test_greedy_scan_stop_list(be_name, n_more):
    """eos_more[0 .. n_eos_more) stop a row exactly as eos does, entries past n_eos_more do not; while pos < min_len every stop token leaves
    the ranking AND the normaliser of the token score; live ones count in it."""
    be = get_backend(be_name)
    V, ldl, eos, pad, max_len, pos = 1000, 1024, 900, 0, 8, 3
    more_all = [33, 640, 950]
    stops = [eos] + more_all[:n_more]
    spare = more_all[n_more] if n_more < 3 else 450
    lg, unf = stop_rows(V, stops, spare)
    more = more_all if n_more else [spare, -1, -1]                # (an id sits in the unused entries: it must be ignored)
    for min_len in (0, pos, pos + 1):
        sup = pos < min_len
        emit, tok, still, top2, sc = ref_step(lg, unf, stops, pad, sup)
        if not sup:
            s = stops[-1]
            assert list(tok) == [s, s - 9, s, s, s, spare, 500] and list(still) == [0, 1, 0, 0, 0, 1, 1]
        else:
            assert not np.isin(tok, stops).any() and list(still) == list(unf) and tok[1] == stops[-1] - 9 and tok[2] == stops[-1] + 11
        o = Outs(be, 7, max_len, unf, top2_cols=0)
        select(be, o, rows=7, V=V, ldl=ldl, logits=be.buf(padded(lg, ldl)), max_len=max_len, pos=pos, eos=eos, pad=pad, more=more, n_more=n_more,
               min_len=min_len)
        assert np.array_equal(get(o.next), emit) and np.array_equal(get(o.out)[:, pos], emit), (get(o.next), emit)
        assert np.array_equal(get(o.unf), still) and int(get(o.n_unf)[0]) == int(still.sum())
        same_bits(get(o.top2), top2, "top2")
        np.testing.assert_allclose(get(o.ts)[:, pos - 1], sc, **TS_TOL)


@pytest.mark.parametrize("be_name", BACKENDS)
def test_greedy_scan_pos_dev_form(be_name):
    """The graph-replay form: the column is *pos_dev + pos, top2 is [max_len][rows][2] indexed by it; nothing else changes.  A column at or
    past max_len writes no out_ids / token_scores element (next_ids and the flags still move)."""
    be = get_backend(be_name)
    V, ldl, eos, max_len, rows = 320, 320, 7, 6, 5
    lg, _ = scan_case(V, 9)
    lg = lg[:rows]
    unf = np.array([1, 1, 0, 1, 1], np.int32)
    emit, _, still, top2, sc = ref_step(lg, unf, [eos], 0, False)
    for base, pos in ((2, 1), (0, 5), (4, 0)):
        col = base + pos
        o = Outs(be, rows, max_len, unf, top2_cols=max_len)
        select(be, o, rows=rows, V=V, ldl=ldl, logits=be.buf(lg), max_len=max_len, pos=pos, pos_dev=be.buf(np.array([base], np.int32)), eos=eos)
        out, ts, t2 = get(o.out), get(o.ts), get(o.top2)
        assert np.array_equal(get(o.next), emit) and np.array_equal(out[:, col], emit) and np.all(np.delete(out, col, 1) == SENT_ID)
        np.testing.assert_allclose(ts[:, col - 1], sc, **TS_TOL)
        assert np.all(np.delete(ts, col - 1, 1) == SENT_TS)
        same_bits(t2[col], top2, "top2[column]")
        assert np.all(np.delete(t2, col, 0) == SENT32)
        assert np.array_equal(get(o.unf), still)
    for base, pos in ((5, 1), (3, 4)):                            # column max_len and beyond (top2 not given: its array ends at max_len)
        o = Outs(be, rows, max_len, unf)
        select(be, o, rows=rows, V=V, ldl=ldl, logits=be.buf(lg), max_len=max_len, pos=pos, pos_dev=be.buf(np.array([base], np.int32)), eos=eos)
        assert np.all(get(o.out) == SENT_ID) and np.all(get(o.ts) == SENT_TS)
        assert np.array_equal(get(o.next), emit) and np.array_equal(get(o.unf), still) and int(get(o.n_unf)[0]) == int(still.sum())


def step_ctr_launches(be, rows, fused_of=None):
    """three launches on the same counters: some rows go on; all rows end; nothing is left.  Returns after each launch
    (c[0], c[1], c[2], c[6], *n_unfinished, unfinished[])."""
    V, ldl, eos, max_len = 320, 320, 7, 8
    a = noise(rows, V, 21)
    a[np.arange(rows), 8 + np.arange(rows) % 300] = WIN
    a[1::3, eos] = WIN + 1                                        # every third row ends in the first launch (rows = 1: none)
    b = noise(rows, V, 22)
    b[:, eos] = WIN
    ctr = be.buf(np.array([-5, -1, 4, 0, 0, 0, 0, 0], np.int32))
    o = Outs(be, rows, max_len, np.ones(rows, np.int32))
    seen = []
    for k, lg in enumerate((a, b, b)):
        kw = dict(rows=rows, V=V, max_len=max_len, pos=1 + k, eos=eos, step_ctr=ctr)
        if fused_of is None:
            select(be, o, ldl=ldl, logits=be.buf(lg), **kw)
        else:
            select(be, o, fused=1, fz=fused_of(lg, [eos]), **kw)
        c = get(ctr)
        seen.append((int(c[0]), int(c[1]), int(c[2]), int(c[6]), int(get(o.n_unf)[0]), get(o.unf)))
    return seen


def check_step_ctr(seen, rows):
    live = rows - len(range(1, rows, 3))
    (c0, c1, c2, c6, nu, unf) = seen[0]
    assert (c0, c1, c2, c6, nu) == (live, -1, 5, 0, 0) and int(unf.sum()) == live
    assert seen[1][:5] == (0, 5, 6, 0, 0) and not seen[1][5].any()       # the step index at which every row had finished
    assert seen[2][:5] == (0, 5, 7, 0, 0)                                # ... recorded once


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("rows", [1, 256])
def test_greedy_scan_step_counters(be_name, rows):
    """step_ctr: the last workgroup to arrive publishes the unfinished count in c[0], records the first all-finished step in c[1] (once),
    advances c[2], and leaves the arrival counter c[6] and *n_unfinished at 0 for the next launch."""
    check_step_ctr(step_ctr_launches(get_backend(be_name), rows), rows)


# =======================================================================================================================================
# B. fused tail
# =======================================================================================================================================
def top_partials(lg, stops, lse=True):
    """TopOut (mg_kernels.h) in numpy: per 32-feature tile {best, second, index of the best (int bits), sum exp(x - best)} over the tile's
    non-stop features ({-3e38, -3e38, 0x7fffffff, 0} for a tile without one); the stop logits apart in stopv[row][k] (unused entries hold
    +1e30 here: reading one would win the row)."""
    rows, V = lg.shape
    nt = (V + 31) // 32
    x = np.full((rows, nt * 32), -np.inf)
    x[:, :V] = lg
    x[:, [s for s in stops if s >= 0]] = -np.inf
    x = x.reshape(rows, nt, 32)
    srt = np.sort(x, axis=2)
    b1, b2 = srt[..., -1], srt[..., -2]
    idx = np.argmax(x, axis=2) + 32 * np.arange(nt)[None, :]
    has = np.isfinite(b1)
    with np.errstate(invalid="ignore"):
        w = np.where(has, np.exp(x - np.where(has, b1, 0.0)[..., None]).sum(2), 0.0)
    p = np.zeros((rows, nt, 4), np.float32)
    p[..., 0] = np.where(has, b1, NEG)
    p[..., 1] = np.where(np.isfinite(b2), b2, NEG)
    p[..., 2] = np.where(has, idx, 0x7fffffff).astype(np.int32).view(np.float32)
    p[..., 3] = w if lse else 0.0
    sv = np.full((rows, 4), PADV, np.float32)
    for k, s in enumerate(stops):
        if s >= 0:
            sv[:, k] = lg[:, s]
    return p, sv


class FusedEnv:
    """embedding table, gain and the activation buffers of the fused tail for `rows` rows of width d"""

    def __init__(self, be, rows, V, d, with_x2, seed=3):
        r = np.random.RandomState(seed)
        self.be, self.rows, self.V, self.d, self.eps = be, rows, V, d, 1e-6
        self.emb = pk.bf16_round((0.2 + r.uniform(0, 3, (V, 1))) * r.standard_normal((V, d)))
        self.gain = (1 + 0.3 * r.standard_normal(d)).astype(np.float32)
        self.EMB, self.GAIN = be.buf(pk.bf16_bits(self.emb)), be.buf(self.gain)
        self.with_x2, self.ld, self.col0 = with_x2, d + 128, 64
        self.Rp = (rows + 31) // 32 * 32

    def fresh(self):
        be = self.be
        self.h = be.buf(np.full((self.rows + 1, self.d), np.nan, np.float32))
        self.x = be.buf(np.full(self.Rp * self.d, NAN16, np.uint16))
        self.x2 = be.buf(np.full(self.Rp * self.ld, SENT16, np.uint16)) if self.with_x2 else None

    def fz(self, lg, stops, lse=True):
        self.fresh()
        p, sv = top_partials(lg, list(stops) + [-1] * (4 - len(stops)), lse)
        return dict(ptop=self.be.buf(p), stopv=self.be.buf(sv), emb=self.EMB, gain=self.GAIN, h=self.h, x_pk=self.x, x2=self.x2,
                    x2_ld=self.ld if self.with_x2 else 0, x2_col0=self.col0 if self.with_x2 else 0, d=self.d, eps=self.eps)

    def check_next_step(self, emit):
        """h = the embedding row of the EMITTED token, x2 window = its bits, x_pk = embed_norm_rows' bits and the float64 RMSNorm; nothing
        outside rows / window is written"""
        be, rows, d = self.be, self.rows, self.d
        h = get(self.h)
        same_bits(h[:rows], self.emb[emit], "h")
        assert np.isnan(h[rows]).all()
        xb = pk.unpack_tile_bits(get(self.x), d)
        assert np.all(xb[rows:] == NAN16)
        h2 = be.buf(np.full((rows, d), np.nan, np.float32))
        x2 = be.buf(np.full(self.Rp * d, NAN16, np.uint16))
        err = be.buf(np.zeros(1, np.int32))
        assert lib_of(be).mgk_embed_norm_rows(be.stream, be.buf(emit.astype(np.int64)).ptr, self.EMB.ptr, h2.ptr, self.GAIN.ptr, x2.ptr, None, 0, 0,
                                              rows, d, self.V, err.ptr, self.eps) == 0
        assert int(get(err)[0]) == 0
        same_bits(xb[:rows], pk.unpack_tile_bits(get(x2), d)[:rows], "x_pk against embed_norm_rows")
        ref, bound = rms_bound(self.emb[emit], self.gain, self.eps)
        assert (np.abs(pk.bf16_to_f32(xb[:rows]) - ref) <= bound + 2.0 ** -8 * np.abs(ref)).all()
        if self.with_x2:
            wb = pk.unpack_tile_bits(get(self.x2), self.ld)
            same_bits(wb[:rows, self.col0:self.col0 + d], pk.bf16_bits(self.emb[emit]), "x2 window")
            assert np.all(wb[rows:] == SENT16) and np.all(wb[:, :self.col0] == SENT16) and np.all(wb[:, self.col0 + d:] == SENT16)


def tile_rows(V):
    """(winner indices, tie pairs) for the fused tail's cut: tile c = features [32c, 32c + 32) belongs to thread c % 256, load (c / 256) % 4
    of batch c / 1024; wave = thread / 64."""
    nt = (V + 31) // 32
    win = [0, V - 1, 32 * min(250, nt - 1) + 5]                    # thread 250: the last wave (where the row has that many tiles)
    ties = [(32 * 2 + 5, 32 * 2 + 9), (32 * 2 + 31, 32 * 3), (32 * 1 + 4, 32 * min(70, nt - 2) + 1)]      # one tile; neighbouring tiles; two waves
    if nt > 256 + 3:
        ties.append((32 * 3 + 7, 32 * (256 + 3) + 2))              # two loads of thread 3
    if nt > 1024:
        win.append(32 * 1024 + 3)                                  # the second batch
        ties.append((32 * 0 + 7, 32 * 1024 + 1))                   # two batches of thread 0
        ties.append((32 * 200 + 1, 32 * 1024 + 30))                # the lower index in the last wave's first batch, the higher in wave 0's second
    return sorted(set(win)), ties


def unfused_run(be, lg, unf, stops, pad, max_len, pos, min_len):
    V = lg.shape[1]
    ldl = (V + 31) // 32 * 32
    o = Outs(be, len(lg), max_len, unf, top2_cols=0)
    select(be, o, rows=len(lg), V=V, ldl=ldl, logits=be.buf(padded(lg, ldl)), max_len=max_len, pos=pos, eos=stops[0], pad=pad, more=stops[1:],
           min_len=min_len)
    return o


def compare_fused(be, env, lg, unf, stops, pad, max_len, pos, min_len, what):
    """one fused launch against the float64 reference and, exactly, against the full-row scan on the same logits"""
    rows, V = lg.shape
    sup = pos < min_len
    emit, _, still, top2, sc = ref_step(lg, unf, stops, pad, sup)
    o = Outs(be, rows, max_len, unf, n_unf=0, top2_cols=0)
    select(be, o, fused=1, rows=rows, V=V, max_len=max_len, pos=pos, eos=stops[0], pad=pad, more=stops[1:], min_len=min_len, fz=env.fz(lg, stops))
    u = unfused_run(be, lg, unf, stops, pad, max_len, pos, min_len)
    assert np.array_equal(get(o.next), emit), (what, get(o.next), emit)
    for a, b, name in ((o.next, u.next, "next_ids"), (o.out, u.out, "out_ids"), (o.unf, u.unf, "unfinished"), (o.n_unf, u.n_unf, "n_unfinished"),
                       (o.top2, u.top2, "top2")):
        same_bits(get(a), get(b), "%s: %s fused against the scan" % (what, name))
    assert np.array_equal(get(o.unf), still)
    same_bits(get(o.top2), top2, "top2")
    ts, tu = get(o.ts), get(u.ts)
    print("%s V=%d fused token score max abs err %.3g" % (what, V, np.abs(ts[:, pos - 1] - sc).max()))
    np.testing.assert_allclose(ts[:, pos - 1], sc, **TS_TOL)
    np.testing.assert_allclose(ts, tu, **TS_TOL)
    assert np.all(np.delete(ts, pos - 1, 1) == SENT_TS) and np.all(ts[np.asarray(unf) == 0, pos - 1] == 0)
    env.check_next_step(emit)
    return emit


def fused_params():
    out = []
    for V in (500, 1000, 32768, 32800, 33201):
        for be in BACKENDS:
            out.append(pytest.param(be.values[0], V, marks=be.marks, id="%s-V%d" % (be.values[0], V)))
    return out


@pytest.mark.parametrize("be_name,V", fused_params())
def test_fused_tail_winner_positions_and_ties(be_name, V):
    """Partials made in numpy (TopOut's format): the winner in the first / last tile, the last wave and the second batch; ties inside a tile,
    between tiles, waves, loads and batches; one row finished.  Ids, flags, count and top2 equal the full-row scan's bit for bit."""
    be = get_backend(be_name)
    win, ties = tile_rows(V)
    rows = len(win) + len(ties) + 2
    lg = noise(rows, V, 200 + V % 89)
    for r, i in enumerate(win):
        lg[r, i] = WIN
    for k, (a, b) in enumerate(ties):
        lg[len(win) + k, [a, b]] = WIN
    lg[-2, 77] = WIN                                               # the finished row
    unf = np.ones(rows, np.int32)
    unf[-2] = 0
    env = FusedEnv(be, rows, V, 64, True)
    emit = compare_fused(be, env, lg, unf, [40], 2, 6, 3, 0, "places")
    assert list(emit[:len(win)]) == win and list(emit[len(win):-2]) == [a for a, _ in ties] and emit[-2] == 2


@pytest.mark.parametrize("be_name,V", [pytest.param("emu", 481), pytest.param("hip", 481, marks=pytest.mark.gpu),
                                       pytest.param("emu", 1000), pytest.param("hip", 33201, marks=pytest.mark.gpu)])
@pytest.mark.parametrize("n_stop", [1, 4])
def test_fused_tail_stop_tokens(be_name, V, n_stop):
    """Stop tokens live in stopv, outside the ranked partials: a stop token ties with a ranked token above / below it, two stop tokens tie,
    a tile holds stop tokens only (V = 481 and 33201 with 4 stop tokens: the last tile is feature V - 1 alone; its .w = 0 adds nothing to
    the normaliser), and
    MinLength takes 1 and 4 stop tokens out of ranking and normaliser."""
    be = get_backend(be_name)
    last = V - 1
    stops = [100] if n_stop == 1 else [100, 300, last, 70]         # (not ascending: stopv's order is the list's, the tie-break is by id)
    s = stops[-1]
    lg = noise(8, V, 300 + n_stop)
    lg[0, last] = WIN                                              # (4 stop tokens) the stop token that is a tile of its own wins
    lg[1, [s - 37, s]] = WIN                                       # ranked token below the stop id
    lg[2, [s, s + 41]] = WIN                                       # stop id below the ranked token
    lg[3, stops] = WIN                                             # all stop tokens tie: the lowest id
    lg[4, s], lg[4, 200] = WIN, WIN - 1
    lg[5, 201] = WIN
    lg[6, s] = WIN                                                 # finished
    lg[7, last - 1] = WIN
    unf = np.array([1, 1, 1, 1, 1, 1, 0, 1], np.int32)
    env = FusedEnv(be, 8, V, 64, False)
    if V % 32 == 1 and n_stop == 4:
        p, _ = top_partials(lg, stops + [-1] * (4 - n_stop))
        assert np.all(p[:, -1, 3] == 0) and np.all(p[:, -1, 0] == NEG)
    emit = compare_fused(be, env, lg, unf, stops, 0, 8, 3, 0, "live")
    assert list(emit) == [last, s - 37, s, min(stops), s, 201, 0, last - 1]
    emit = compare_fused(be, env, lg, unf, stops, 0, 8, 3, 4, "suppressed")
    assert not np.isin(emit[unf == 1], stops).any() and emit[4] == 200 and emit[1] == s - 37 and emit[2] == s + 41


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("with_x2", [False, True])
@pytest.mark.parametrize("d", [64, 1024, 2048])
def test_fused_tail_next_step_activations(be_name, d, with_x2):
    """h / x_pk / x2 for the next step at the widths the models have: the emitted token's embedding row (pad for the finished row), x_pk
    bit-equal to mgk_embed_norm_rows on the emitted ids (the kernel's NOTE on its summation order), the x2 window alone written."""
    be = get_backend(be_name)
    V, rows = 500, 37
    lg = noise(rows, V, 400 + d)
    where = np.random.RandomState(d).randint(0, V, rows)
    lg[np.arange(rows), where] = WIN
    unf = np.ones(rows, np.int32)
    unf[[4, 36]] = 0
    env = FusedEnv(be, rows, V, d, with_x2)
    emit = compare_fused(be, env, lg, unf, [int(where[9])], 11, 6, 2, 0, "d=%d" % d)
    assert emit[4] == 11 and emit[36] == 11 and emit[9] == where[9]


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("rows", [1, 256])
def test_fused_tail_step_counters(be_name, rows):
    """the step_ctr bookkeeping of the fused tail: the full-row scan's, launch for launch"""
    be = get_backend(be_name)
    env = FusedEnv(be, rows, 320, 64, False)
    seen = step_ctr_launches(be, rows, fused_of=env.fz)
    check_step_ctr(seen, rows)
    ref = step_ctr_launches(be, rows)
    for a, b in zip(seen, ref):
        assert a[:5] == b[:5] and np.array_equal(a[5], b[5])


@pytest.mark.parametrize("be_name", BACKENDS)
def test_fused_tail_on_lm_head_partials(be_name):
    """The same comparison with the partials the lm_head launch leaves (mgk_lm_head_step, lse = 1, two stop tokens) instead of numpy's."""
    be = get_backend(be_name)
    lib = lib_of(be)
    M, V, K, stops, max_len, pos = 40, 500, 128, [1, 333], 8, 3
    r = np.random.RandomState(12)
    x, w = r.standard_normal((M, K)).astype(np.float32), (0.3 * r.standard_normal((V, K))).astype(np.float32)
    nt = (V + 31) // 32
    P, ptop, stopv = be.zeros((M, nt * 32), np.float32), be.zeros((M, nt, 4), np.float32), be.buf(np.full((M, 4), PADV, np.float32))
    stop4 = (C.c_int * 4)(stops[0], stops[1], -1, -1)
    assert lib.mgk_lm_head_step(be.stream, be.buf(pk.pack_tiles(x)).ptr, be.buf(pk.pack_tiles(w)).ptr, P.ptr, M, V, K, nt * 32, None, 0, 0.0, 0.0,
                                ptop.ptr, stopv.ptr, C.cast(stop4, C.c_void_p), 1, 1) == 0
    lg = get(P)[:, :V]
    unf = np.ones(M, np.int32)
    unf[5] = 0
    env = FusedEnv(be, M, V, 64, True)
    for min_len in (0, 6):
        emit, _, still, top2, sc = ref_step(lg, unf, stops, 0, pos < min_len)
        fz = env.fz(lg, stops)
        fz["ptop"], fz["stopv"] = ptop, stopv
        o = Outs(be, M, max_len, unf, top2_cols=0)
        select(be, o, fused=1, rows=M, V=V, max_len=max_len, pos=pos, eos=stops[0], more=stops[1:], min_len=min_len, fz=fz)
        u = unfused_run(be, lg, unf, stops, 0, max_len, pos, min_len)
        # (random logits: a row's margin is whatever it is, but both kernels and the reference rank the SAME float32 values: still decided)
        assert np.array_equal(get(o.next), emit) and np.array_equal(get(u.next), emit)
        assert np.array_equal(get(o.unf), still) and int(get(o.n_unf)[0]) == int(still.sum())
        same_bits(get(o.top2), top2, "top2")
        same_bits(get(o.top2), get(u.top2), "top2 against the scan")
        np.testing.assert_allclose(get(o.ts)[:, pos - 1], sc, **TS_TOL)
        np.testing.assert_allclose(get(o.ts), get(u.ts), **TS_TOL)
        env.check_next_step(emit)


# =======================================================================================================================================
# the slot table: a model written from the comments of SlotTable / slot_refill (mg_kernels.h) and the counters layout (engine.hip)
# =======================================================================================================================================
class SlotModel:
    """`slots` decode rows work through a queue of sequences, nsamp per image.  A slot holds: img (the sequence, -1 = idle), pos (position
    of the token fed to the step, 0 = the first), pool (K/V entry of the sequence's image = image % pool_cap), next (token fed next), live.
    ctr: [0] live slots after the last refill, [1] sequences finished, [2] refills run, [4] queue head (sequences), [5] images ready,
    [7] oldest live sequence, or the head when nothing is live."""

    def __init__(self, slots, nseq, max_len, pool_cap, start_id, stops, nsamp=1, first_tok=None, ready=0):
        self.S, self.N, self.T, self.cap, self.start, self.stops, self.nsamp, self.first = slots, nseq, max_len, pool_cap, start_id, list(stops), nsamp, first_tok
        self.img = np.full(slots, -1, np.int32)
        self.pos = np.full(slots, 55, np.int32)                    # idle slots hold whatever they held: a sentinel here
        self.pool = np.full(slots, 66, np.int32)
        self.next = np.full(slots, SENT_ID, np.int64)
        self.unf = np.zeros(slots, np.int32)
        self.out_len = np.full(nseq, -3, np.int32)
        self.out = np.full((nseq, max_len), SENT_ID, np.int64)
        self.ctr = np.zeros(16, np.int32)
        self.ctr[[3, 6]] = 77                                      # unused by the queue: must stay
        self.ctr[5] = ready

    def select(self, toks):
        """toks[slot] = the token selected for a live slot: written at column pos + 1 of its sequence; a stop token or the last column ends it"""
        for r in range(self.S):
            if not self.unf[r]:
                continue
            q, col = int(self.img[r]), int(self.pos[r]) + 1
            self.next[r], self.pos[r] = toks[r], col
            if col < self.T:
                self.out[q, col] = toks[r]
            if int(toks[r]) in self.stops or col + 1 >= self.T:
                self.unf[r], self.img[r] = 0, -1
                self.out_len[q] = min(col + 1, self.T)
                self.ctr[1] += 1

    def refill(self):
        """idle slots, in slot order, take the next sequences whose image is ready; with first_tok a sequence whose prefill token is a stop
        token (or max_len 1) is finished with one column and never takes a slot"""
        head, ready = int(self.ctr[4]), int(self.ctr[5]) * self.nsamp
        for r in range(self.S):
            while not self.unf[r] and head < ready:
                q = head
                head += 1
                tok = self.start
                if self.first is not None:
                    tok = int(self.first[q])
                    if tok in self.stops or self.T <= 1:
                        self.out_len[q] = 1
                        self.ctr[1] += 1
                        continue
                self.img[r], self.pool[r], self.pos[r], self.next[r], self.unf[r] = q, (q // self.nsamp) % self.cap, 0, tok, 1
        live = self.img[self.unf == 1]
        self.ctr[4], self.ctr[0], self.ctr[7] = head, len(live), live.min() if len(live) else head
        self.ctr[2] += 1


class SlotDev:
    """the device side of a SlotModel: the same arrays as buffers, and the mgk_slot_table over them"""

    def __init__(self, be, m):
        self.be, self.m = be, m
        self.pos, self.img, self.pool, self.ctr, self.out_len = (be.buf(a) for a in (m.pos, m.img, m.pool, m.ctr, m.out_len))
        self.next, self.unf, self.out = be.buf(m.next), be.buf(m.unf), be.buf(m.out)
        self.first = be.buf(np.asarray(m.first, np.int64)) if m.first is not None else None
        t = SlotTab()
        t.pos, t.img, t.pool, t.ctr, t.out_len = self.pos.ptr, self.img.ptr, self.pool.ptr, self.ctr.ptr, self.out_len.ptr
        t.pool_cap, t.start_id, t.first_tok, t.n_stop, t.max_len, t.nsamp = m.cap, m.start, ptr(self.first), len(m.stops), m.T, m.nsamp
        for k in range(4):
            t.stop[k] = m.stops[k] if k < len(m.stops) else -1
        self.tab = t

    def refill(self, expect=0):
        assert lib_of(self.be).mgk_slot_refill(self.be.stream, C.byref(self.tab), self.next.ptr, self.unf.ptr, self.m.S) == expect

    def check(self, what):
        m = self.m
        for name in ("img", "pos", "pool", "next", "unf", "out_len", "out", "ctr"):
            got, exp = get(getattr(self, name)), getattr(m, name)
            assert np.array_equal(got, exp), "%s: %s\n got %s\n exp %s" % (what, name, got.tolist(), exp.tolist())


# =======================================================================================================================================
# C. queue form, one launch
# =======================================================================================================================================
QUEUE_IMG = [4, -1, 0, 9, 2, -1]
QUEUE_POS = [2, 55, 0, 4, 6, 55]


def queue_model(order, max_len=8, stops=(7,), nseq=10):
    """6 slots holding sequences out of order at different positions, two idle; `order` permutes which slot holds what"""
    m = SlotModel(6, nseq, max_len, 4, 1, stops, ready=nseq)
    for r, s in enumerate(order):
        m.img[r], m.pos[r] = QUEUE_IMG[s], QUEUE_POS[s]
        m.unf[r] = int(QUEUE_IMG[s] >= 0)
        m.pool[r] = QUEUE_IMG[s] % 4 if QUEUE_IMG[s] >= 0 else 66
    m.ctr[[0, 1, 2, 4, 7]] = [4, 3, 12, 10, 0]
    return m


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("order", [[0, 1, 2, 3, 4, 5], [3, 5, 4, 1, 0, 2]], ids=["order0", "order1"])
def test_queue_greedy_select_one_launch(be_name, order):
    """The `stream` branch of greedy_select_kernel: a live slot writes column pos + 1 of ITS sequence (token and score), a stop token of the
    list (past min_len) or the last column frees the slot; idle slots - NaN logits - touch nothing.  Sequence 0 is below min_len (its stop
    token is suppressed), sequence 9 above it (it ends), sequence 2 reaches the last column, sequence 4 goes on."""
    be = get_backend(be_name)
    V, ldl, max_len, stops, min_len = 1000, 1024, 8, [7, 500, 900], 3
    m = queue_model(order, max_len, stops)
    per_seq = {4: noise(1, V, 54)[0], 0: noise(1, V, 50)[0], 9: noise(1, V, 59)[0], 2: noise(1, V, 52)[0]}
    per_seq[4][[123, 640]] = WIN                                   # a tie on the way
    per_seq[0][900], per_seq[0][31] = WIN, WIN - 1                 # column 1 < min_len: the stop token is out
    per_seq[9][900], per_seq[9][31] = WIN, WIN - 1                 # column 5: it ends the sequence
    per_seq[2][999] = WIN                                          # column 7 = the last
    lg = np.full((6, V), np.nan, np.float32)
    toks, sc = np.zeros(6, np.int64), {}
    for r in range(6):
        q = int(m.img[r])
        if q >= 0:
            lg[r] = per_seq[q]
            col = int(m.pos[r]) + 1
            _, t, _, _, s = ref_step(lg[r:r + 1], [1], stops, 0, col < min_len)
            toks[r], sc[q] = t[0], (col, s[0])
    assert [int(toks[list(m.img).index(q)]) for q in (4, 0, 9, 2)] == [123, 31, 900, 999]
    dev = SlotDev(be, m)
    o = Outs(be, 6, max_len, m.unf, n_unf=13, nseq=m.N)
    o.next, o.out, o.unf = dev.next, dev.out, dev.unf
    select(be, o, rows=6, V=V, ldl=ldl, logits=be.buf(padded(lg, ldl)), max_len=max_len, pos=0, eos=stops[0], more=stops[1:],
           min_len=min_len, slots=dev.tab)
    m.select(toks)
    dev.check("queue greedy")
    assert list(m.out_len[[9, 2]]) == [6, 8] and m.ctr[1] == 5 and list(np.sort(m.img)) == [-1, -1, -1, -1, 0, 4]
    assert int(get(o.n_unf)[0]) == 13                              # the queue form does not count
    ts = get(o.ts)
    exp = np.full(ts.shape, SENT_TS, np.float32)
    for q, (col, s) in sc.items():
        np.testing.assert_allclose(ts[q, col - 1], s, **TS_TOL)
        exp[q, col - 1] = ts[q, col - 1]
    same_bits(ts, exp, "token_scores outside (sequence, column)")


def sample_call(be, queue, lg, V, ldl, eos, min_len, T, top_k, top_p, seed, sids, o, max_len, pos=0, tab=None, rows=None):
    lib = lib_of(be)
    rows = len(lg) if rows is None else rows
    sb = be.buf(np.asarray(sids, np.uint64).view(np.int64)) if sids is not None else None
    args = [be.stream, be.buf(lg).ptr, rows, V, ldl, eos, 0, min_len, T, top_k, top_p, seed, ptr(sb), o.next.ptr, o.out.ptr, max_len, pos,
            o.unf.ptr, o.n_unf.ptr, ptr(o.ts), max(max_len - 1, 1)]
    return lib.mgk_sample_select_queue(*args, C.byref(tab)) if queue else lib.mgk_sample_select(*args)


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("top_k,top_p", [(0, 1.0), (40, 0.9)], ids=["plain", "topk-topp"])
@pytest.mark.parametrize("with_sids", [False, True], ids=["seq-index", "stream-ids"])
@pytest.mark.parametrize("V", [1000, 8000, 33201])
def test_queue_sample_select_against_batch_form(be_name, V, with_sids, top_k, top_p):
    """sample_select_kernel<.., QUEUE = true> (V = 1000 / 8000 / 33201: the three instantiations) on the 6-slot table, in two slot orders:
    every live slot's token and score are bit-equal to a one-row batch-form launch at the sequence's stream and the slot's column - the draw
    depends on the sequence's place in the queue, never on the slot - and the slot bookkeeping is the model's.  Sequence 0 (column 1) is
    below min_len and sequence 9 above it, both with EOS far ahead; sequence 2 reaches the last column."""
    be = get_backend(be_name)
    ldl, max_len, eos, min_len, T, seed = (V + 31) // 32 * 32, 8, 7, 3, 0.8, 0x1234ABCD5678
    sids = (np.arange(10, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(5)) if with_sids else None
    per_seq = {q: noise(1, V, 70 + q)[0] * 2 for q in (4, 0, 9, 2)}
    per_seq[0][eos] = per_seq[9][eos] = 30.0                       # EOS holds all the mass wherever it is allowed
    batch = {}
    for q, col in ((4, 3), (0, 1), (9, 5), (2, 7)):                # the batch form: one row, stream of the sequence, the slot's column
        o = Outs(be, 1, max_len, [1])
        assert sample_call(be, False, padded(per_seq[q][None], ldl), V, ldl, eos, min_len, T, top_k, top_p, seed,
                           [sids[q] if with_sids else q], o, max_len, pos=col) == 0
        batch[q] = (int(get(o.next)[0]), get(o.ts)[0, col - 1], col)
        assert int(get(o.out)[0, col]) == batch[q][0]
    assert batch[9][0] == eos and batch[0][0] != eos
    for order in ([0, 1, 2, 3, 4, 5], [3, 5, 4, 1, 0, 2]):
        m = queue_model(order, max_len, [eos])
        lg = np.full((6, ldl), np.nan, np.float32)
        toks = np.zeros(6, np.int64)
        for r in range(6):
            if m.img[r] >= 0:
                lg[r] = padded(per_seq[int(m.img[r])][None], ldl)[0]
                toks[r] = batch[int(m.img[r])][0]
        dev = SlotDev(be, m)
        o = Outs(be, 6, max_len, m.unf, n_unf=13, nseq=m.N)
        o.next, o.out, o.unf = dev.next, dev.out, dev.unf
        assert sample_call(be, True, lg, V, ldl, eos, min_len, T, top_k, top_p, seed, sids, o, max_len, tab=dev.tab) == 0
        m.select(toks)
        dev.check("queue sampled, order %s" % order)
        assert int(get(o.n_unf)[0]) == 13
        ts = get(o.ts)
        exp = np.full(ts.shape, SENT_TS, np.float32)
        for q, (_, s, col) in batch.items():
            exp[q, col - 1] = s
        same_bits(ts, exp, "token_scores")


# =======================================================================================================================================
# D. slot_refill, and a scripted queue run
# =======================================================================================================================================
def refill_and_check(be, m, what):
    dev = SlotDev(be, m)
    dev.refill()
    m.refill()
    dev.check(what)
    return dev


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("rows", [1, 64, 65, 256])
def test_slot_refill_single_launches(be_name, rows):
    """slot_refill against the model on 1 .. 256 slots (the kernel's LDS arrays hold 256): nothing ready; fewer ready than idle slots; a table
    half live (every other slot) with more ready than idle; a second launch with nothing to do moves ctr[2] alone."""
    be = get_backend(be_name)
    N = 2 * rows + 5
    m = SlotModel(rows, N, 6, 300, 1, [7], ready=0)                # empty table, nothing ready: ctr[7] = head
    m.ctr[4] = 3
    dev = refill_and_check(be, m, "empty")
    assert m.ctr[7] == 3 and m.ctr[0] == 0 and np.all(m.img == -1)
    ready = max(1, rows // 2)
    m.ctr[5], m.ctr[4] = ready, 0                                  # ready < the queue and (rows > 1) < the idle slots
    upload(dev.ctr, m.ctr)
    dev.refill()
    m.refill()
    dev.check("partly ready")
    assert m.ctr[4] == ready and m.ctr[0] == min(ready, rows) and m.ctr[7] == 0
    for r in range(0, rows, 2):                                    # every other slot ends; the whole queue is ready
        if m.unf[r]:
            m.unf[r], m.img[r] = 0, -1
    m.ctr[5] = N
    for name in ("unf", "img", "ctr"):
        upload(getattr(dev, name), getattr(m, name))
    dev.refill()
    m.refill()
    dev.check("refill between live slots")
    assert m.ctr[0] == rows and np.all(m.unf == 1)
    before = m.ctr.copy()
    dev.refill()
    m.refill()
    dev.check("nothing to do")
    before[2] += 1
    assert np.array_equal(m.ctr, before)


@pytest.mark.parametrize("be_name", BACKENDS)
def test_slot_refill_samples_per_image_and_pool_wrap(be_name):
    """nsamp = 3: the ready counter counts images, head / img / done count sequences; pool = (sequence / 3) % pool_cap with pool_cap = 2, so
    image 2 wraps to entry 0.  2 images ready of 4: 6 sequences may start."""
    be = get_backend(be_name)
    m = SlotModel(8, 12, 6, 2, 1, [7], nsamp=3, ready=2)
    dev = refill_and_check(be, m, "2 images ready")
    assert list(m.img) == [0, 1, 2, 3, 4, 5, -1, -1] and list(m.pool[:6]) == [0, 0, 0, 1, 1, 1] and m.ctr[4] == 6
    m.unf[[0, 1, 2, 4]], m.img[[0, 1, 2, 4]] = 0, -1
    m.ctr[5] = 4
    for name in ("unf", "img", "ctr"):
        upload(getattr(dev, name), getattr(m, name))
    dev.refill()
    m.refill()
    dev.check("4 images ready")
    assert list(m.img) == [6, 7, 8, 3, 9, 5, 10, 11] and list(m.pool) == [0, 0, 0, 1, 1, 1, 1, 1] and m.ctr[7] == 3 and m.ctr[4] == 12


@pytest.mark.parametrize("be_name", BACKENDS)
def test_slot_refill_first_tokens(be_name):
    """first_tok (the OCR queue): sequences whose prefill token is a stop token never take a slot (out_len 1, counted as done) - the first
    three in a row here, then one between live ones; max_len = 1 finishes every ready sequence at once."""
    be = get_backend(be_name)
    stops = [7, 500, 900]
    first = [900, 7, 500, 41, 42, 7, 43, 44, 45]
    m = SlotModel(3, 9, 6, 8, 1, stops, first_tok=first, ready=8)
    refill_and_check(be, m, "first tokens")
    assert list(m.img) == [3, 4, 6] and list(m.next) == [41, 42, 43] and list(m.out_len[[0, 1, 2, 5]]) == [1, 1, 1, 1]
    assert m.ctr[1] == 4 and m.ctr[4] == 7 and m.ctr[7] == 3
    m = SlotModel(3, 9, 1, 8, 1, stops, first_tok=first, ready=6)
    refill_and_check(be, m, "max_len 1")
    assert np.all(m.img == -1) and m.ctr[1] == 6 and m.ctr[4] == 6 and m.ctr[0] == 0 and m.ctr[7] == 6 and list(m.out_len[:6]) == [1] * 6


def script_logits(m, script, V, seed):
    """for every live slot a row of small noise with a large value at the sequence's scripted token of this step; NaN for idle slots"""
    lg = np.full((m.S, V), np.nan, np.float32)
    toks = np.zeros(m.S, np.int64)
    for r in range(m.S):
        if m.unf[r]:
            q, p = int(m.img[r]), int(m.pos[r])
            toks[r] = script[q][p] if p < len(script[q]) else 20 + (q + p) % 10
            lg[r] = noise(1, V, seed + r)[0]
            lg[r, toks[r]] = 30.0
    return lg, toks


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("form", ["greedy", "greedy-first-tok", "sampled"])
def test_scripted_queue_run(be_name, form):
    """A whole queue run of select + refill per step on scripted logits: 7 sequences over 3 slots (sampled: 3 images x 3 samples over 3 slots,
    a pool of 2), max_len 6, sequences that stop at their first step, mid-way, or never (max_len ends them); the ready counter is raised in
    two stages.  After every step the whole slot state equals the model's; at the end the outputs are the scripts."""
    be = get_backend(be_name)
    V, ldl, max_len, eos = 320, 320, 6, 7
    sampled = form == "sampled"
    stops = [eos] if sampled else [eos, 300]
    script = [[31, 32, eos], [eos], [33, 34, 35, 36, 37, 38], [300 if not sampled else eos], [41, 42, 43, 44, eos], [51, eos], [61, 62, 63, 64, 65, 66]]
    first = None
    if sampled:
        script += [[71, 72, 73, eos], [eos]]
    N, nsamp, cap = len(script), (3 if sampled else 1), 2 if sampled else 4
    if form == "greedy-first-tok":
        first = [90, eos, 91, 300, 300, 92, 93]                    # sequences 1, 3, 4 began with a stop token: no slot, no step
    m = SlotModel(3, N, max_len, cap, 1, stops, nsamp=nsamp, first_tok=first, ready=1 if sampled else 3)
    dev = SlotDev(be, m)
    dev.refill()                                                   # the first sequences take their slots
    m.refill()
    dev.check("first refill")
    o = Outs(be, 3, max_len, m.unf, nseq=N, scores=False)
    o.next, o.out, o.unf = dev.next, dev.out, dev.unf
    L = be.buf(np.zeros((3, ldl), np.float32))
    steps = 0
    while m.ctr[0] > 0 or m.ctr[4] < N:
        assert steps < 60
        if steps == 2:                                             # the rest of the queue becomes ready (stream_chunk_done_kernel's add)
            m.ctr[5] = N // nsamp
            c = get(dev.ctr)
            c[5] = N // nsamp
            upload(dev.ctr, c)
        assert np.array_equal(get(dev.img), m.img) and np.array_equal(get(dev.pos), m.pos)
        lg, toks = script_logits(m, script, V, 1000 + 10 * steps)
        upload(L, lg)
        if sampled:
            assert sample_call(be, True, lg, V, ldl, eos, 0, 1.0, 1, 1.0, 99, None, o, max_len, tab=dev.tab) == 0
        else:
            select(be, o, rows=3, V=V, ldl=ldl, logits=L, max_len=max_len, pos=0, eos=eos, more=stops[1:], slots=dev.tab)
        m.select(toks)
        dev.check("step %d select" % steps)
        dev.refill()
        m.refill()
        dev.check("step %d refill" % steps)
        steps += 1
    out, out_len, c = get(dev.out), get(dev.out_len), get(dev.ctr)
    assert c[1] == c[4] == N and c[0] == 0 and c[7] == N and c[2] == steps + 1 and not get(dev.unf).any() and np.all(get(dev.img) == -1)
    for q in range(N):
        if first is not None and first[q] in stops:
            assert out_len[q] == 1 and np.all(out[q] == SENT_ID)
            continue
        n = next((i + 1 for i, t in enumerate(script[q]) if t in stops), max_len)
        n = min(n, max_len - 1)                                    # columns 1 .. n hold the script; max_len ends a sequence that never stops
        assert out_len[q] == n + 1, (q, out_len[q], n)
        assert list(out[q, 1:n + 1]) == script[q][:n] and out[q, 0] == SENT_ID and np.all(out[q, n + 1:] == SENT_ID)


# =======================================================================================================================================
# E. argument checks
# =======================================================================================================================================
@pytest.mark.parametrize("be_name", BACKENDS)
def test_selection_entries_validate(be_name):
    """Every rejected call returns before anything is launched; the accepted ones at the end run on one zeroed buffer large enough for each role."""
    be = get_backend(be_name)
    lib = lib_of(be)
    one = be.zeros((4096,), np.int64)
    p = one.ptr

    def desc(**kw):
        d = SelDesc()
        d.logits = d.next_ids = d.out_ids = d.unfinished = d.n_unfinished = p
        d.rows, d.V, d.ldl, d.max_len, d.pos, d.eos = 1, 8, 8, 4, 1, 1
        for k, v in kw.items():
            if k.startswith("slots_"):
                setattr(d.slots, k[6:], v)
            else:
                setattr(d, k, v)
        return lib.mgk_select_ex(be.stream, C.byref(d))

    fused = dict(fused=1, ptop=p, stopv=p, ntiles=1, tok_emb=p, gain=p, h=p, x_pk=p, d=64)
    assert lib.mgk_select_ex(be.stream, None) == MG_E_ARG
    for f in ("logits", "next_ids", "out_ids", "unfinished", "n_unfinished"):
        assert desc(**{f: None}) == MG_E_ARG, f
    for f in ("ptop", "stopv", "tok_emb", "gain", "h", "x_pk"):
        assert desc(**{**fused, f: None}) == MG_E_ARG, f
    assert desc(rows=0) == MG_E_SHAPE and desc(rows=257) == MG_E_SHAPE
    assert desc(ldl=4) == MG_E_SHAPE and desc(V=6, ldl=6) == MG_E_SHAPE
    assert desc(n_eos_more=-1) == MG_E_ARG and desc(n_eos_more=4) == MG_E_ARG
    assert desc(**{**fused, "d": 2056}) == MG_E_SHAPE and desc(**{**fused, "d": 60}) == MG_E_SHAPE and desc(**{**fused, "d": 72}) == MG_E_SHAPE
    assert desc(**{**fused, "ntiles": 2}) == MG_E_SHAPE
    assert desc(**{**fused, "x2_pk": p, "x2_ld": 96, "x2_col0": 40}) == MG_E_SHAPE                    # the window leaves its buffer
    assert desc(**fused, slots_pos=p, slots_img=p, slots_ctr=p, slots_out_len=p) == MG_E_ARG           # no queue form of the fused tail
    assert desc(slots_pos=p) == MG_E_ARG                                                              # a slot table without img / ctr / out_len
    assert desc(token_scores=p, ts_ld=2) == MG_E_SHAPE
    assert desc() == 0 and desc(**fused) == 0                                                         # the accepted forms do run

    def tab(**kw):
        t = SlotTab()
        t.pos = t.img = t.pool = t.ctr = t.out_len = p
        t.pool_cap, t.nsamp, t.max_len = 2, 1, 4
        for k, v in kw.items():
            setattr(t, k, v)
        return t

    def refill(t, rows=1, nxt=p, unf=p):
        return lib.mgk_slot_refill(be.stream, C.byref(t) if t is not None else None, nxt, unf, rows)

    assert refill(None) == MG_E_ARG and refill(tab(), nxt=None) == MG_E_ARG and refill(tab(pool=None)) == MG_E_ARG
    assert refill(tab(), rows=257) == MG_E_SHAPE and refill(tab(), rows=0) == MG_E_SHAPE
    assert refill(tab(nsamp=0)) == MG_E_ARG and refill(tab(pool_cap=0)) == MG_E_ARG and refill(tab(n_stop=5)) == MG_E_ARG
    assert refill(tab()) == 0

    def sampleq(t, rows=1, V=8, ldl=8, T=1.0, top_k=0, top_p=1.0, lg=p):
        return lib.mgk_sample_select_queue(be.stream, lg, rows, V, ldl, 1, 0, 0, T, top_k, top_p, 1, None, p, p, 4, 0, p, p, None, 0,
                                           C.byref(t) if t is not None else None)

    assert sampleq(None) == MG_E_ARG and sampleq(tab(img=None)) == MG_E_ARG and sampleq(tab(), lg=None) == MG_E_ARG
    assert sampleq(tab(), ldl=4) == MG_E_ARG and sampleq(tab(), V=6, ldl=6) == MG_E_ARG and sampleq(tab(), rows=0) == MG_E_ARG
    assert sampleq(tab(), T=0.0) == MG_E_ARG and sampleq(tab(), top_k=-1) == MG_E_ARG
    assert sampleq(tab(), rows=257) == MG_E_SHAPE
    assert sampleq(tab(), V=36868, ldl=36868) == MG_E_UNSUPPORTED
