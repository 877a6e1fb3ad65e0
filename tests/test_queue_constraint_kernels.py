"""The queue forms of the selection step under a decoder prompt and a constraint, at operator level (include/mgrapher.h
mgk_select_queue_ex, mgk_sample_select_queue_ex, mgk_slot_refill_ex, mgk_beam_step_queue_ex, mgk_beam_slots_step_ex), on scripted logits.

Greedy and sampled stream branch: 5 slots, one idle, V = 70 with a row stride of 96.  The free rows are compared with the PLAIN queue
operator (mgk_select_ex with a slot table / mgk_sample_select_queue) on the same logits with the disallowed entries set to -inf on the host:
tokens exactly, token scores bit for bit.  The forced row, the empty-set row and the idle row follow the contract: a forced column writes
the prompt's token - EOS here - scores 0.0, keeps the slot and the state; the empty-set row emits EOS, scores 0.0, FREES its slot, moves to
the sink and is counted; the idle row (NaN logits, a stale but valid state) writes nothing.  The slot bookkeeping is tests/
test_selection_step.py's SlotModel.
slot_refill: the state and the first prompt token of the image handed over, a bad first id counted and replaced; with no prompt and no
constraint byte-identical to mgk_slot_refill.
Beam queue: three images with their own prompts and start states through two slots of K = 3 rows, so one slot is handed over; per image
bit for bit against the BATCH operators (mgk_beam_init_constrained / mgk_beam_step_constrained / mgk_beam_finalize, themselves pinned on
tests/constraint_script.py and tests/prompt_script.py in tests/test_constraint_kernels.py)."""
import ctypes as C

import numpy as np
import pytest

from markushgrapher_amd.engine import MgkConstraint
from tests import constraint_script
from tests.backends import get_backend
from tests.beam_script import Script, tie_free
from tests.test_beam_kernels import EOS as BEOS, NAN_PAD, START, Logits, _read, _write, er_mid
from tests.test_constraint_kernels import beam_automaton, beam_con_lib, run_beam_con
from tests.test_decoder_prompt_kernels import beam_prompts
from tests.test_selection_step import (BACKENDS, SENT_ID, SENT_TS, Outs, SlotDev, SlotModel, SlotTab, get, lib_of, noise, padded, same_bits,
                                       sample_call, select)

MG_E_ARG = -2
V, LDL, MAX_LEN, MIN_LEN, EOS, SINK = 70, 96, 8, 4, 7, 3
SEQ = [6, 2, -1, 9, 4]            # the sequence in every slot, -1 = idle; nsamp = 2: images 3, 1, -, 4, 2
POS = [2, 1, 55, 0, 6]            # column written = pos + 1: 3, 2, -, 1, 7 (the last)
NSAMP = 2
# token classes: 0 other, 1 EOS, 2 the tokens {10 .. 19}, 3 the tokens {20 .. 29}
CLS = np.zeros(V, np.int64)
CLS[EOS], CLS[10:20], CLS[20:30] = 1, 2, 3
#                other EOS  10s  20s
TABLE = np.array([[0, SINK, 1, -1],        # state 0: everything but the 20s
                  [-1, SINK, 2, 0],        # state 1: EOS, the 10s, the 20s
                  [-1, SINK, -1, -1],      # state 2: EOS only
                  [-1, SINK, -1, -1]], np.int64)      # the sink
STATE = [0, 1, 1, 2, 1]           # slot 2 is idle: its state is stale, and valid
# prompts per IMAGE (5 images): image 1 (slot 1, column 2) is inside its prompt of 3 tokens, whose column 2 is EOS
PROMPT = np.array([[1, 0, 0], [1, 33, EOS], [1, 40, 0], [1, 0, 0], [1, 0, 0]], np.int64)
PLEN = [1, 3, 2, 1, 1]


class QueueCon(C.Structure):
    _fields_ = [("prompt_ids", C.c_void_p), ("prompt_len", C.c_void_p), ("prompt_ld", C.c_int), ("V", C.c_int), ("bad", C.c_void_p),
                ("con", C.POINTER(MgkConstraint)), ("con_start", C.c_void_p)]


def q_lib(be):
    lib, P, I, F = lib_of(be), C.c_void_p, C.c_int, C.c_float
    lib.mgk_select_queue_ex.argtypes = [P, P, P]
    lib.mgk_sample_select_queue_ex.argtypes = [P, P, I, I, I, I, I, I, F, I, F, C.c_uint64, P, P, P, I, P, P, I, P, P]
    lib.mgk_slot_refill_ex.argtypes = [P, P, P, P, I, P, P, I]
    return lib


class Con:
    """device side of the constraint and the prompt of one launch"""

    def __init__(self, be, rows_state, starts=None, prompt=True, con=True):
        cp = np.zeros(LDL, np.uint16)
        cp[:V] = CLS
        self.CLS, self.TAB = be.buf(cp), be.buf(np.ascontiguousarray(TABLE, np.int32))
        self.STATE, self.EMPTY, self.BAD = be.buf(np.asarray(rows_state, np.int32)), be.buf(np.zeros(1, np.int32)), be.buf(np.zeros(1, np.int32))
        self.P, self.LEN = be.buf(PROMPT), be.buf(np.asarray(PLEN, np.int32))
        self.START = be.buf(np.asarray(starts if starts is not None else [0] * len(PLEN), np.int32))
        self.con = MgkConstraint(self.CLS.ptr, self.TAB.ptr, TABLE.shape[0], TABLE.shape[1], self.STATE.ptr, self.EMPTY.ptr)
        self.q = QueueCon()
        if prompt:
            self.q.prompt_ids, self.q.prompt_len, self.q.prompt_ld, self.q.V, self.q.bad = self.P.ptr, self.LEN.ptr, PROMPT.shape[1], V, self.BAD.ptr
        if con:
            self.q.con, self.q.con_start = C.pointer(self.con), self.START.ptr


def stream_case():
    """-> (SlotModel, raw logits [5][V], host-masked logits).  Slot 0 (sequence 6, column 3, state 0): a token of the 20s wins the raw logits
    and is masked - an allowed 10s token is next; slot 1: a forced column; slot 2: idle, NaN logits; slot 3 (column 1 < MIN_LEN, state 2 =
    EOS only): the empty set; slot 4 (column 7, the last, state 1): free, a 20s token wins and is allowed."""
    m = SlotModel(5, 10, MAX_LEN, 4, 1, [EOS], nsamp=NSAMP, ready=5)
    for r in range(5):
        m.img[r], m.pos[r], m.unf[r] = SEQ[r], POS[r], int(SEQ[r] >= 0)
        m.pool[r] = (SEQ[r] // NSAMP) % 4 if SEQ[r] >= 0 else 66
    m.ctr[[0, 1, 2, 4, 7]] = [4, 3, 12, 10, 2]
    lg = noise(5, V, 91)
    lg[0, 25], lg[0, 12] = 6.0, 5.0
    lg[1, 50] = 6.0
    lg[2] = np.nan
    lg[3, 40] = 6.0
    lg[4, 22], lg[4, EOS] = 6.0, 5.5
    masked = lg.copy()
    for r in (0, 4):
        masked[r, TABLE[STATE[r]][CLS] < 0] = -np.inf
    return m, lg, masked


def expected(m, toks):
    """the contract on the SlotModel: free rows as SlotModel.select; the forced row keeps its slot whatever the token; the empty-set row
    ends on EOS"""
    t = np.array(toks, np.int64)
    t[1], t[3] = PROMPT[SEQ[1] // NSAMP, POS[1] + 1], EOS
    assert t[1] == EOS
    keep = (m.img[1], m.unf[1])
    m.select(t)
    # SlotModel.select ended slot 1 on its EOS: a forced EOS does not end the row
    q = int(keep[0])
    m.img[1], m.unf[1] = keep
    m.out_len[q] = -3
    m.ctr[1] -= 1
    state = np.array(STATE)
    state[0], state[3], state[4] = TABLE[0, CLS[t[0]]], SINK, TABLE[1, CLS[t[4]]]
    return t, state


@pytest.mark.parametrize("be_name", BACKENDS)
def test_greedy_stream_branch(be_name):
    be = get_backend(be_name)
    lib = q_lib(be)
    m, lg, masked = stream_case()
    # the plain queue operator on the masked logits: tokens and scores of the free rows
    ref_m, _, _ = stream_case()
    ref_dev = SlotDev(be, ref_m)
    ro = Outs(be, 5, MAX_LEN, ref_m.unf, nseq=ref_m.N)
    ro.next, ro.out, ro.unf = ref_dev.next, ref_dev.out, ref_dev.unf
    select(be, ro, rows=5, V=V, ldl=LDL, logits=be.buf(padded(masked, LDL)), max_len=MAX_LEN, pos=0, eos=EOS, min_len=MIN_LEN, slots=ref_dev.tab)
    ref_next, ref_ts = get(ro.next), get(ro.ts)
    assert ref_next[0] == 12 and ref_next[4] == 22, ref_next
    dev = SlotDev(be, m)
    c = Con(be, STATE)
    o = Outs(be, 5, MAX_LEN, m.unf, n_unf=13, nseq=m.N)
    o.next, o.out, o.unf = dev.next, dev.out, dev.unf
    from tests.test_selection_step import SelDesc
    d = SelDesc()
    raw = be.buf(padded(lg, LDL))
    d.logits, d.rows, d.V, d.ldl, d.eos, d.pad = raw.ptr, 5, V, LDL, EOS, 0
    for k in range(3):
        d.eos_more[k] = -1
    d.next_ids, d.out_ids, d.max_len, d.min_len = o.next.ptr, o.out.ptr, MAX_LEN, MIN_LEN
    d.unfinished, d.n_unfinished, d.token_scores, d.ts_ld, d.slots = o.unf.ptr, o.n_unf.ptr, o.ts.ptr, MAX_LEN - 1, dev.tab
    assert lib.mgk_select_queue_ex(be.stream, C.byref(d), C.byref(c.q)) == 0
    toks, state = expected(m, ref_next)
    dev.check("greedy queue under prompt and constraint")
    assert np.array_equal(get(c.STATE), state), (get(c.STATE), state)
    assert int(get(c.EMPTY)[0]) == 1 and int(get(c.BAD)[0]) == 0 and int(get(o.n_unf)[0]) == 13
    assert m.img[3] == -1 and m.out_len[9] == 2 and m.img[1] == 2 and m.img[4] == -1 and m.out_len[4] == MAX_LEN
    ts = get(o.ts)
    exp = np.full(ts.shape, SENT_TS, np.float32)
    exp[6, 2], exp[4, 6] = ref_ts[6, 2], ref_ts[4, 6]           # free rows: the plain operator's bits on the masked row
    exp[2, 1], exp[9, 0] = 0.0, 0.0                             # the forced column and the empty set score 0.0
    same_bits(ts, exp, "token scores")
    # without a slot table the operator refuses; the plain operators keep refusing a queue with a constraint (tests/test_constraint_kernels.py)
    d.slots = SlotTab()
    assert lib.mgk_select_queue_ex(be.stream, C.byref(d), C.byref(c.q)) == MG_E_ARG


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("top_k,top_p", [(0, 1.0), (12, 0.9)], ids=["plain", "topk-topp"])
def test_sampled_stream_branch(be_name, top_k, top_p):
    be = get_backend(be_name)
    lib = q_lib(be)
    T, seed = 0.8, 0x1234ABCD5678
    m, lg, masked = stream_case()
    ref_m, _, _ = stream_case()
    ref_dev = SlotDev(be, ref_m)
    ro = Outs(be, 5, MAX_LEN, ref_m.unf, nseq=ref_m.N)
    ro.next, ro.out, ro.unf = ref_dev.next, ref_dev.out, ref_dev.unf
    assert sample_call(be, True, padded(masked, LDL), V, LDL, EOS, MIN_LEN, T, top_k, top_p, seed, None, ro, MAX_LEN, tab=ref_dev.tab) == 0
    ref_next, ref_ts = get(ro.next), get(ro.ts)
    assert TABLE[0, CLS[ref_next[0]]] >= 0 and TABLE[1, CLS[ref_next[4]]] >= 0
    dev = SlotDev(be, m)
    c = Con(be, STATE)
    o = Outs(be, 5, MAX_LEN, m.unf, n_unf=13, nseq=m.N)
    o.next, o.out, o.unf = dev.next, dev.out, dev.unf
    raw = be.buf(padded(lg, LDL))
    assert lib.mgk_sample_select_queue_ex(be.stream, raw.ptr, 5, V, LDL, EOS, 0, MIN_LEN, T, top_k, top_p, seed, None, o.next.ptr,
                                          o.out.ptr, MAX_LEN, o.unf.ptr, o.ts.ptr, MAX_LEN - 1, C.byref(dev.tab), C.byref(c.q)) == 0
    toks, state = expected(m, ref_next)
    dev.check("sampled queue under prompt and constraint")
    assert np.array_equal(get(c.STATE), state), (get(c.STATE), state)
    assert int(get(c.EMPTY)[0]) == 1 and int(get(c.BAD)[0]) == 0
    ts = get(o.ts)
    exp = np.full(ts.shape, SENT_TS, np.float32)
    exp[6, 2], exp[4, 6] = ref_ts[6, 2], ref_ts[4, 6]
    exp[2, 1], exp[9, 0] = 0.0, 0.0
    same_bits(ts, exp, "token scores")


def _refill_case(nsamp):
    m = SlotModel(5, 12, MAX_LEN, 4, 1, [EOS], nsamp=nsamp, ready=5)
    m.img[:], m.unf[:] = [3, -1, -1, 5, -1], [1, 0, 0, 1, 0]
    m.pos[[0, 3]], m.pool[[0, 3]] = [2, 4], [(3 // nsamp) % 4, (5 // nsamp) % 4]
    m.ctr[[0, 1, 2, 4, 7]] = [2, 4, 9, 6, 3]
    return m


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("nsamp", [1, 2])
def test_slot_refill_sets_state_and_first_prompt_token(be_name, nsamp):
    """slots 1, 2 and 4 are idle and take sequences 6, 7, 8: images 6, 7, 8 with one sequence per image, images 3, 3, 4 with two.  Each gets
    its IMAGE's first prompt id (next_ids and column 0 of its output row) and start state; the first ids of images 4 and 7 are outside the
    vocabulary: replaced by 0 and counted.  Live slots and their states are untouched."""
    be = get_backend(be_name)
    lib = q_lib(be)
    m = _refill_case(nsamp)
    m.ctr[5] = 9 if nsamp == 1 else 5                             # images ready: sequences [6, 9) are handed out either way
    n_img = 9
    first = np.array([11, 12, 13, 14, V + 5, 16, 17, -2, 19], np.int64)
    starts = np.array([0, 1, 2, 1, 2, 0, 1, 2, 0], np.int32)
    dev = SlotDev(be, m)
    cp = np.zeros(LDL, np.uint16)
    CLSB, TAB = be.buf(cp), be.buf(np.ascontiguousarray(TABLE, np.int32))
    ST, EMPTY, BAD = be.buf(np.full(5, SINK, np.int32)), be.buf(np.zeros(1, np.int32)), be.buf(np.zeros(1, np.int32))
    pid = np.full((n_img, 2), 5, np.int64)
    pid[:, 0] = first
    PID, LEN, START_ST = be.buf(pid), be.buf(np.full(n_img, 2, np.int32)), be.buf(starts)
    con = MgkConstraint(CLSB.ptr, TAB.ptr, TABLE.shape[0], TABLE.shape[1], ST.ptr, EMPTY.ptr)
    q = QueueCon()
    q.prompt_ids, q.prompt_len, q.prompt_ld, q.V, q.bad, q.con, q.con_start = PID.ptr, LEN.ptr, 2, V, BAD.ptr, C.pointer(con), START_ST.ptr
    out = be.buf(np.full((m.N, MAX_LEN), SENT_ID, np.int64))
    assert lib.mgk_slot_refill_ex(be.stream, C.byref(dev.tab), dev.next.ptr, dev.unf.ptr, 5, C.byref(q), out.ptr, MAX_LEN) == 0
    m.refill()
    owners = {r: int(m.img[r]) // nsamp for r in (1, 2, 4)}
    assert sorted(int(m.img[r]) for r in (1, 2, 4)) == [6, 7, 8]
    want_state, want_out, bad = np.full(5, SINK, np.int32), np.full((m.N, MAX_LEN), SENT_ID, np.int64), 0
    for r, im in owners.items():
        tok = int(first[im])
        if tok < 0 or tok >= V:
            tok, bad = 0, bad + 1
        m.next[r] = tok
        want_state[r] = starts[im]
        want_out[int(m.img[r]), 0] = tok
    dev.check("refill under prompt and constraint")
    assert np.array_equal(get(ST), want_state) and np.array_equal(get(out), want_out)
    assert int(get(BAD)[0]) == bad and bad == 1, (bad, owners)


@pytest.mark.parametrize("be_name", BACKENDS)
def test_slot_refill_null_fields_is_the_plain_operator(be_name):
    be = get_backend(be_name)
    lib = q_lib(be)
    a, b = SlotDev(be, _refill_case(2)), SlotDev(be, _refill_case(2))
    a.refill()
    for q in (None, C.byref(QueueCon())):
        b = SlotDev(be, _refill_case(2))
        assert lib.mgk_slot_refill_ex(be.stream, C.byref(b.tab), b.next.ptr, b.unf.ptr, 5, q, None, 0) == 0
        for name in ("img", "pos", "pool", "next", "unf", "out_len", "out", "ctr"):
            assert np.array_equal(get(getattr(a, name)).view(np.uint8), get(getattr(b, name)).view(np.uint8)), name
    m = _refill_case(2)
    m.refill()
    a.m = m
    a.check("plain refill")


# ---- beam queue ------------------------------------------------------------------------------------------------------------------------
def bq_lib(be):
    lib, P, I, F = beam_con_lib(be), C.c_void_p, C.c_int, C.c_float
    lib.mgk_beam_step_queue_ex.argtypes = [P, P, P, I, I, I, I, I, P, I, I, F, I, P, P, P, P, P, P, P]
    lib.mgk_beam_slots_step_ex.argtypes = [P, P, I, I, I, I, I, I, I] + [P] * 8 + [I, I, P, P, P, P, I, I, P, P, P]
    return lib


def run_beam_queue(be, ref, aut, N, slots, K, max_length, prompts, ready, min_length=0, length_penalty=1.0, early_stopping=False, num_return=1, pad=0):
    """tests/test_beam_kernels.run_queue with the _ex operators: beam_step (slots) -> reorder (slots) -> slots_step (end first)"""
    lib = bq_lib(be)
    script = ref["script"]
    Vb, R = script.V, slots * K
    ldl, T_cap = Vb + 14, max_length - 1
    lens = [len(p) for p in prompts]
    ld = max(lens) + 1
    pid = np.full((N, ld), Vb + 100, np.int64)
    for b, p in enumerate(prompts):
        pid[b, :len(p)] = p
    PID, LEN, BAD = be.buf(pid), be.buf(np.asarray(lens, np.int32)), be.buf(np.zeros(1, np.int32))
    CLSB, TAB = be.buf(aut.cls), be.buf(aut.table)
    ST, EMPTY, START_ST = be.buf(np.zeros(R, np.int32)), be.buf(np.zeros(1, np.int32)), be.buf(np.asarray(ref["starts"], np.int32))
    con = MgkConstraint(CLSB.ptr, TAB.ptr, aut.n_states, aut.n_classes, ST.ptr, EMPTY.ptr)
    q = QueueCon()
    q.prompt_ids, q.prompt_len, q.prompt_ld, q.V, q.bad, q.con, q.con_start = PID.ptr, LEN.ptr, ld, Vb, BAD.ptr, C.pointer(con), START_ST.ptr
    state = be.zeros(lib.mgk_beam_state_bytes(slots, K, max_length), np.uint8)
    pos, img, pool, live = be.zeros(R, np.int32), be.buf(np.full(R, -1, np.int32)), be.zeros(R, np.int32), be.zeros(R, np.int32)
    bpool, assign = be.zeros(slots, np.int32), be.buf(np.full(slots, -1, np.int32))
    nid, bidx, ctr = be.buf(np.full(R, START, np.int64)), be.zeros(R, np.int32), be.zeros(16, np.int32)
    anc = be.zeros((T_cap, R), np.int32)
    nr = num_return
    out_ids = be.buf(np.full((N * nr, max_length), pad, np.int64))
    out_len, out_sc = be.zeros(N, np.int32), be.zeros(N * nr, np.float32)
    obi, ots = be.zeros((N * nr, max_length - 1), np.int32), be.zeros((N * nr, max_length - 1), np.float32)
    div = be.buf(np.array([lib.mgk_beam_length_divisor(c, length_penalty) for c in range(max_length + 1)], np.float32))
    lg = Logits(be, R, Vb, ldl, NAN_PAD)
    s = be.stream
    prefixes = [None] * R
    h_live, h_img = np.zeros(R, np.int32), np.full(R, -1, np.int32)
    slot_of, inits = {}, 0
    for step in range(N * max_length + 8):
        c = _read(be, ctr)
        c[5] = ready(step)
        _write(be, ctr, c)
        lg.set({r: script.logits(int(h_img[r]), prefixes[r]) for r in range(R) if h_live[r]})
        assert lib.mgk_beam_step_queue_ex(s, be.p(state), be.p(lg.dev), ldl, Vb, slots, K, max_length, be.p(div), BEOS, min_length,
                                          C.c_float(length_penalty), int(early_stopping), be.p(nid), be.p(bidx), be.p(ctr), be.p(pos), be.p(live),
                                          be.p(img), C.byref(q)) == 0
        assert lib.mgk_beam_reorder_anc(s, be.p(anc), be.p(bidx), R, max_length - 1, None, be.p(ctr), be.p(pos), be.p(live)) == 0
        n, bi = _read(be, nid), _read(be, bidx)
        old = [None if prefixes[r] is None else (prefixes[bi[r]] + [int(n[r])]) for r in range(R)]
        st_after = _read(be, ST)
        for r in range(R):                                        # the states follow the beams: the automaton over what each row now holds
            if h_live[r]:
                assert st_after[r] == script.state(int(h_img[r]), old[r]), ("state", step, r)
        assert lib.mgk_beam_slots_step_ex(s, be.p(state), slots, K, max_length, pad, BEOS, START, int(early_stopping), be.p(pos), be.p(img),
                                          be.p(pool), be.p(bpool), be.p(live), be.p(assign), be.p(nid), be.p(anc), T_cap, 4, be.p(out_ids),
                                          be.p(out_len), be.p(out_sc), be.p(ctr), 1, nr, be.p(obi), be.p(ots), C.byref(q)) == 0
        n = _read(be, nid)
        p_live, p_img, p_pos, st_now = _read(be, live), _read(be, img), _read(be, pos), _read(be, ST)
        prefixes = [None] * R
        for r in range(R):
            if p_live[r] and h_live[r] and p_img[r] == h_img[r]:
                prefixes[r] = old[r]
            elif p_live[r]:
                # slot init under prompt and start state: the image's first prompt token is fed, position 0, its start state in the K rows
                i = int(p_img[r])
                prefixes[r] = [int(prompts[i][0])]
                assert n[r] == prompts[i][0] and p_pos[r] == 0 and st_now[r] == ref["starts"][i], (step, r, i)
                slot_of.setdefault(i, r // K)
                inits += 1
        h_live, h_img = p_live, p_img
        if _read(be, ctr)[1] == N:
            break
    assert inits == N * K and int(_read(be, BAD)[0]) == 0
    return dict(out_ids=_read(be, out_ids), out_len=_read(be, out_len), scores=_read(be, out_sc), beam_indices=_read(be, obi),
                token_scores=_read(be, ots), slot_of=slot_of)


BEAM_Q = [("bans", [2, 1, 3], dict(num_return=2)), ("few", [1, 3, 2], dict(num_return=2, length_penalty=0.7, early_stopping=True))]


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("case", BEAM_Q, ids=[c[0] for c in BEAM_Q])
def test_beam_queue_across_hand_over(be_name, case):
    """3 images, 2 slots, K = 3, V = 500, max_length 10: image 2 is handed the slot of whichever image stops first, with its own prompt (of
    another length) and start state.  n-best ids, sequence scores, token scores and beam indices (numbered image * K) equal the batch
    operators' bit for bit; forced columns hold the image's beam-0 row and 0.0."""
    kind, lens, o = case
    be = get_backend(be_name)
    N, K, ml, Vb = 3, 3, 10, 500
    aut = beam_automaton(kind, Vb)
    prompts = beam_prompts(lens, Vb)
    _, ref = tie_free(lambda seed: Script(Vb, BEOS, seed=seed, eos_rank=er_mid, n_hot=20),
                      lambda s: constraint_script.beam_reference(s, aut, N, K, ml, prompts, **o))
    nr = o["num_return"]
    batch = run_beam_con(be, ref, aut, N, K, ml, prompts, False, **o)
    qd = run_beam_queue(be, ref, aut, N, 2, K, ml, prompts, ready=lambda step: min(N, 2 + step // 2), **o)
    assert sorted(qd["slot_of"]) == [0, 1, 2] and qd["slot_of"][2] in (0, 1), qd["slot_of"]
    for i in range(N):
        rows = slice(i * nr, (i + 1) * nr)
        assert np.array_equal(qd["out_ids"][rows], batch["out_ids"][rows]), ("ids", i, qd["out_ids"][rows], batch["out_ids"][rows])
        assert np.array_equal(qd["beam_indices"][rows], batch["beam_indices"][rows]), ("beam indices", i)
        assert np.array_equal(qd["scores"][rows].view(np.uint32), batch["scores"][rows].view(np.uint32)), ("scores", i)
        assert np.array_equal(qd["token_scores"][rows].view(np.uint32), batch["token_scores"][rows].view(np.uint32)), ("token scores", i)
        n_i = int((ref["beam_indices"][rows] != -1).sum(axis=1).max())
        assert qd["out_len"][i] == 1 + n_i
        if lens[i] > 1:
            assert np.all(qd["beam_indices"][i * nr, :lens[i] - 1] == i * K) and np.all(qd["token_scores"][i * nr, :lens[i] - 1] == 0.0)
