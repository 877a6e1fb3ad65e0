"""The constraint at operator level (include/mgrapher.h mgk_select_constrained, mgk_sample_select_constrained), on scripted logits.

A whole call runs column by column on the launch's own state (unfinished flags, step counters, the rows' automaton states).  Every column
is compared with the UNCONSTRAINED kernel on the same logits with the disallowed entries set to -inf on the host: ids, next ids,
unfinished flags and step counters exactly, token scores and top2 bit for bit (adding exp(-inf) = 0 in the same order changes no bit).
The states are the test's own: table[state][cls[token]] for a live row in a free column, untouched for a forced or a finished row, the
sink for a row whose allowed set is empty - that row emits EOS, ends, scores 0.0 and raises the counter.  The automata here are raw
tables (C = 1 and C = 2 cannot hold TokenAutomaton's conventions): the kernels know classes and entries only.

Beam search: see the section at the end of the file."""
import ctypes as C

import numpy as np
import pytest

from tests.backends import get_backend
from tests.test_selection_step import BACKENDS, NEG, SENT32, SENT_ID, Outs, SelDesc, get, lib_of, noise, padded, ptr, same_bits, select, upload

MG_E_ARG = -2
EOS, PAD, LO, MAX_LEN, MIN_LEN = 7, 3, 20, 8, 4
WIN = np.float32(5.0)


from markushgrapher_amd.engine import MgkConstraint             # noqa: E402


def con_lib(be):
    lib, P, I, F = lib_of(be), C.c_void_p, C.c_int, C.c_float
    lib.mgk_select_constrained.argtypes = [P, P, P, P, P, I, I, P]
    lib.mgk_sample_select_constrained.argtypes = [P, P, I, I, I, I, I, I, F, I, F, C.c_uint64, P, P, P, I, I, P, P, P, P, P, I, P, P, P, P, I, I, P]
    return lib


# ---- the automata ----------------------------------------------------------------------------------------------------------------------
def automaton(kind, V):
    """-> (cls [V], table [S][C], start states to cycle through).  With singleton classes for EOS and LO the table ends in three placed
    states: S - 3 allows only LO (the logits' loser) and returns to state 0, S - 2 allows only EOS, S - 1 is the sink."""
    r = np.random.RandomState(11)
    if kind == "C1":              # one class: states 0 and 1 allow everything and alternate, state 2 allows nothing
        return np.zeros(V, np.int64), np.array([[1], [0], [-1]]), [0, 1, 2, 1, 0]
    if kind == "C2":              # even / odd tokens: state 0 allows the even ones, state 1 everything, state 2 the odd ones (EOS = 7 among them)
        return np.arange(V) % 2, np.array([[1, -1], [0, 2], [-1, 0]]), [0, 1, 2, 0, 1]
    cls = np.arange(V) if kind == "single" else np.minimum(np.arange(V) % 4096 + (np.arange(V) >= 4096) * 50, 4095)
    Cn = V if kind == "single" else 4096
    assert (cls == EOS).sum() == 1 and (cls == LO).sum() == 1
    S = 7
    table = np.where(r.rand(S, Cn) < 0.5, -1, r.randint(0, S - 3, (S, Cn)))
    table[:, EOS] = np.where(r.rand(S) < 0.5, -1, S - 1)
    table[0, EOS] = -1                                            # (a state in which EOS is disallowed, placed)
    table[1, EOS] = S - 1
    table[S - 3], table[S - 2], table[S - 1] = -1, -1, -1
    table[S - 3, LO] = 0
    table[S - 2, EOS] = table[S - 1, EOS] = S - 1
    return cls, table, [0, S - 3, S - 2, 1, 2, 3]


def allowed_of(cls, table, s):
    return table[s][cls] >= 0


def case_logits(rows, V, col, seed, cls, table, states, min_len):
    """noise with LO the loser of every row, then by row: a disallowed token wins the raw logits (EOS if it is disallowed), an exact tie of
    a disallowed token with an allowed one of higher index, EOS far ahead, or noise alone"""
    lg = noise(rows, V, seed + 31 * col)
    lg[:, LO] = -3.0
    for i in range(rows):
        ok = allowed_of(cls, table, states[i]).copy()
        if col < min_len:
            ok[EOS] = False
        yes, no = np.nonzero(ok)[0], np.nonzero(~ok)[0]
        kind = (i + col) % 4
        if kind == 0 and no.size and yes.size:
            lg[i, EOS if not ok[EOS] else no[0]] = WIN + 1
            if yes[-1] != LO:
                lg[i, yes[-1]] = WIN
        elif kind == 1 and no.size and yes.size and yes[-1] > no[0] and yes[-1] != LO:
            lg[i, no[0]] = lg[i, yes[-1]] = WIN                   # the lowest index of the maximum is disallowed
        elif kind == 2:
            lg[i, EOS] = WIN + 2
    return lg


class Run:
    """the test's model of a call: states, unfinished flags, the counter"""

    def __init__(self, be, rows, V, ldl, cls, table, starts, lens=None, group=1):
        self.be, self.rows, self.V, self.ldl, self.cls, self.table = be, rows, V, ldl, cls, table
        self.state = np.array([starts[r % len(starts)] for r in range(rows)], np.int32)
        self.unf = np.ones(rows, np.int32)
        self.n_empty, self.done_step = 0, -1
        cp = np.zeros(ldl, np.uint16)
        cp[:V] = cls
        self.CLS, self.TAB = be.buf(cp), be.buf(np.ascontiguousarray(table, np.int32))
        self.STATE, self.EMPTY = be.buf(self.state.copy()), be.buf(np.zeros(1, np.int32))
        self.con = MgkConstraint(self.CLS.ptr, self.TAB.ptr, table.shape[0], table.shape[1], self.STATE.ptr, self.EMPTY.ptr)
        self.lens, self.group = lens, group
        if lens is not None:
            ld = max(lens)
            pr = np.random.RandomState(3).randint(8, V, (len(lens), ld)).astype(np.int64)
            pr[:, 0] = 1
            self.prompts, self.ld = pr, ld
            self.P, self.LEN, self.BAD = be.buf(pr), be.buf(np.asarray(lens, np.int32)), be.buf(np.zeros(1, np.int32))
        self.ctr = be.buf(np.array([rows, -1, 0, 0, 0, 0, 0, 0], np.int32))

    def prompt_args(self):
        if self.lens is None:
            return (None, None, 0, 0, None)
        return (self.P.ptr, self.LEN.ptr, self.ld, self.group, self.BAD.ptr)

    def column(self, col, lg, min_len):
        """-> (masked logits for the unconstrained kernel, forced rows, rows with an empty allowed set)"""
        ok = np.stack([allowed_of(self.cls, self.table, s) for s in self.state])
        forced = np.array([self.lens is not None and col < self.lens[r // self.group] for r in range(self.rows)])
        okm = ok.copy()
        if col < min_len:
            okm[:, EOS] = False
        empty = ~okm.any(1) & (self.unf == 1) & ~forced
        masked = np.where(ok | empty[:, None], lg, -np.inf).astype(np.float32)      # (an empty row's reference launch is not looked at)
        return masked, forced, empty

    def advance(self, col, ref_next, ref_unf, forced, empty):
        """the model's column from the unconstrained kernel's -> (emitted ids, unfinished flags); states and counter move"""
        emit, still = ref_next.copy(), ref_unf.copy()
        for r in range(self.rows):
            if forced[r]:
                emit[r], still[r] = self.prompts[r // self.group, col], 1
            elif empty[r]:
                emit[r], still[r] = EOS, 0
                self.state[r] = self.table.shape[0] - 1
                self.n_empty += 1
            elif self.unf[r]:
                nxt = self.table[self.state[r], self.cls[emit[r]]]
                assert nxt >= 0, "the reference emitted a disallowed token"
                self.state[r] = nxt
        if still.sum() == 0 and self.done_step < 0:
            self.done_step = col - 1
        self.unf = still
        return emit, still

    def check_counters(self, col, o):
        c = get(self.ctr)
        got = (int(c[0]), int(c[1]), int(c[2]), int(c[6]), int(get(o.n_unf)[0]))
        assert got == (int(self.unf.sum()), self.done_step, col, 0, 0), (col, got)
        assert np.array_equal(get(self.STATE), self.state), (col, get(self.STATE), self.state)
        assert int(get(self.EMPTY)[0]) == self.n_empty


def run_greedy(be, kind, V, ldl, rows, dev_pos, lens=None, cols=MAX_LEN):
    lib = con_lib(be)
    cls, table, starts = automaton(kind, V)
    m = Run(be, rows, V, ldl, cls, table, starts, lens)
    o = Outs(be, rows, MAX_LEN, m.unf, top2_cols=MAX_LEN if dev_pos else 0)
    upload(o.ts, np.zeros((rows, MAX_LEN - 1), np.float32))
    seen = dict(empty=0, forced=0, finished=0, masked_winner=0, eos_masked=0)
    for col in range(1, cols):
        lg = case_logits(rows, V, col, 400, cls, table, m.state, MIN_LEN)
        masked, forced, empty = m.column(col, lg, MIN_LEN)
        live = (m.unf == 1) & ~forced & ~empty
        seen["masked_winner"] += int((masked.argmax(1) != lg.argmax(1))[live].sum())
        seen["eos_masked"] += int(((lg.argmax(1) == EOS) & (masked[:, EOS] == -np.inf))[live].sum())
        s = Outs(be, rows, MAX_LEN, m.unf, top2_cols=0)
        select(be, s, rows=rows, V=V, max_len=MAX_LEN, pos=col, eos=EOS, logits=be.buf(padded(masked, ldl)), ldl=ldl, pad=PAD, min_len=MIN_LEN)
        d = SelDesc()
        d.logits, d.rows, d.V, d.ldl, d.eos, d.pad = be.buf(padded(lg, ldl)).ptr, rows, V, ldl, EOS, PAD
        for k in range(3):
            d.eos_more[k] = -1
        d.next_ids, d.out_ids, d.max_len, d.min_len = o.next.ptr, o.out.ptr, MAX_LEN, MIN_LEN
        d.pos, d.pos_dev = (1, m.ctr.ptr + 8) if dev_pos else (col, None)
        d.unfinished, d.n_unfinished, d.top2, d.step_ctr = o.unf.ptr, o.n_unf.ptr, o.top2.ptr, m.ctr.ptr
        d.token_scores, d.ts_ld = o.ts.ptr, MAX_LEN - 1
        was = m.unf.copy()
        assert lib.mgk_select_constrained(be.stream, C.byref(d), C.byref(m.con), *m.prompt_args()) == 0
        emit, still = m.advance(col, get(s.next), get(s.unf), forced, empty)
        assert np.array_equal(get(o.next), emit) and np.array_equal(get(o.out)[:, col], emit), (col, get(o.next), emit)
        assert np.array_equal(get(o.unf), still), col
        m.check_counters(col, o)
        ts, top2 = get(o.ts)[:, col - 1], get(o.top2)
        top2 = top2[col] if dev_pos else top2
        cmp = ~forced & ~empty
        same_bits(ts[cmp], get(s.ts)[cmp, col - 1], "token scores against the unconstrained kernel, column %d" % col)
        same_bits(top2[cmp], get(s.top2)[cmp], "top2 against the unconstrained kernel, column %d" % col)
        assert np.all(ts[forced | empty] == 0)
        seen["empty"] += int(empty.sum())
        seen["forced"] += int(forced.sum())
        seen["finished"] += int((was == 0).sum())
    assert np.all(get(o.out)[:, 0] == SENT_ID)
    return seen, m


GREEDY = [("C1", 37, 40), ("C2", 37, 40), ("single", 37, 40), ("C4096", 4100, 4128)]


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("dev_pos", [False, True], ids=["pos", "pos_dev"])
@pytest.mark.parametrize("kind,V,ldl", GREEDY, ids=[g[0] for g in GREEDY])
def test_greedy_scan(be_name, kind, V, ldl, dev_pos):
    """V = 37 / ldl = 40 (a partial last float4) with C = 1, 2 and singleton classes, V = 4100 (more than one load per thread) with
    C = 4096; 6 rows through 7 columns.  The run must have met: a winner of the raw logits that is masked, finished rows, and - with
    singleton classes - a masked winning EOS, the state that allows only the loser, and the EOS-only state below min_len (empty set)."""
    seen, m = run_greedy(get_backend(be_name), kind, V, ldl, 6, dev_pos)
    assert seen["finished"] > 0 and (seen["masked_winner"] > 0 or kind == "C1"), seen
    if kind in ("single", "C4096"):
        assert seen["empty"] == 1 and seen["eos_masked"] > 0, seen             # the row started in the EOS-only state, once
    if kind == "C1":
        assert seen["empty"] == 1                                              # the row started in the state that allows nothing


@pytest.mark.parametrize("be_name", BACKENDS)
def test_greedy_scan_only_the_loser(be_name):
    """one column: a row in the state that allows only LO, the minimum of its logits, emits it and moves to the entry's state (0)"""
    be = get_backend(be_name)
    seen, m = run_greedy(be, "single", 37, 40, 2, False, cols=2)
    assert m.state[1] == 0 and int(get(m.STATE)[1]) == 0                       # row 1 started in S - 3


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("dev_pos", [False, True], ids=["pos", "pos_dev"])
def test_greedy_scan_under_a_prompt(be_name, dev_pos):
    """prompt lengths [1, 3, 5, 2, 4, 1]: a forced column writes the prompt's token and leaves the row's state untouched (the run compares
    the state array after every column); row 2 sits in the EOS-only state through its prompt and meets the empty set at its first free
    column, column 5, where min_len = 4 no longer suppresses EOS - so it emits EOS there by the table, not by the empty rule"""
    seen, m = run_greedy(get_backend(be_name), "single", 37, 40, 6, dev_pos, lens=[1, 3, 5, 2, 4, 1])
    assert seen["forced"] == 0 + 2 + 4 + 1 + 3 + 0 and seen["empty"] == 0


@pytest.mark.gpu
def test_greedy_scan_full_vocabulary():
    """V = 33201 with 2 rows: 8.1 loads per thread, 4096 classes"""
    seen, m = run_greedy(get_backend("hip"), "C4096", 33201, 33216, 2, True)
    assert seen["masked_winner"] > 0


# ---- sampled selection -----------------------------------------------------------------------------------------------------------------
def run_sampled(be, kind, V, ldl, rows, dev_pos, lens=None, cols=MAX_LEN, top_k=12, top_p=0.9):
    lib = con_lib(be)
    cls, table, starts = automaton(kind, V)
    m = Run(be, rows, V, ldl, cls, table, starts, lens)
    seed, T = 0x1234567, 0.8
    sids = be.buf((1000 + 17 * np.arange(rows)).astype(np.uint64).view(np.int64))
    o = Outs(be, rows, MAX_LEN, m.unf, top2_cols=MAX_LEN if dev_pos else 0)
    upload(o.ts, np.zeros((rows, MAX_LEN - 1), np.float32))
    seen = dict(empty=0, forced=0, finished=0)
    for col in range(1, cols):
        lg = case_logits(rows, V, col, 70, cls, table, m.state, MIN_LEN)
        masked, forced, empty = m.column(col, lg, MIN_LEN)
        mb = be.buf(padded(masked, ldl))
        s = Outs(be, rows, MAX_LEN, m.unf)
        assert lib.mgk_sample_select(be.stream, mb.ptr, rows, V, ldl, EOS, PAD, MIN_LEN, T, top_k, top_p, seed, sids.ptr, s.next.ptr, s.out.ptr,
                                     MAX_LEN, col, s.unf.ptr, s.n_unf.ptr, s.ts.ptr, MAX_LEN - 1) == 0
        g = Outs(be, rows, MAX_LEN, m.unf, top2_cols=0)            # top2 of the processed logits: the greedy scan's on the same masked row
        select(be, g, rows=rows, V=V, max_len=MAX_LEN, pos=col, eos=EOS, logits=mb, ldl=ldl, pad=PAD, min_len=MIN_LEN)
        was = m.unf.copy()
        assert lib.mgk_sample_select_constrained(be.stream, be.buf(padded(lg, ldl)).ptr, rows, V, ldl, EOS, PAD, MIN_LEN, T, top_k, top_p, seed,
                                                 sids.ptr, o.next.ptr, o.out.ptr, MAX_LEN, 1 if dev_pos else col,
                                                 m.ctr.ptr + 8 if dev_pos else None, o.unf.ptr, o.n_unf.ptr, m.ctr.ptr, o.ts.ptr, MAX_LEN - 1,
                                                 o.top2.ptr, C.byref(m.con), *m.prompt_args()) == 0
        emit, still = m.advance(col, get(s.next), get(s.unf), forced, empty)
        assert np.array_equal(get(o.next), emit) and np.array_equal(get(o.out)[:, col], emit), (col, get(o.next), emit)
        assert np.array_equal(get(o.unf), still), col
        m.check_counters(col, o)
        ts, top2 = get(o.ts)[:, col - 1], get(o.top2)
        top2 = top2[col] if dev_pos else top2
        cmp = ~forced & ~empty
        same_bits(ts[cmp], get(s.ts)[cmp, col - 1], "scores against the unconstrained kernel, column %d" % col)
        live = cmp & (was == 1)
        same_bits(top2[live], get(g.top2)[live], "top2 against the scan of the masked row, column %d" % col)
        assert np.all(ts[forced | empty] == 0)
        seen["empty"] += int(empty.sum())
        seen["forced"] += int(forced.sum())
        seen["finished"] += int((was == 0).sum())
    return seen, m


SAMPLED = [("C1", 37, 40), ("C2", 37, 40), ("single", 37, 40), ("C4096", 4100, 4128), ("C4096", 33201, 33216)]


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("dev_pos", [False, True], ids=["pos", "pos_dev"])
@pytest.mark.parametrize("kind,V,ldl", SAMPLED, ids=["%s-%d" % g[:2] for g in SAMPLED])
def test_sampled_selection(be_name, kind, V, ldl, dev_pos):
    """5 rows; V = 37, 4100 and 33201 are the kernel's three thread / load configurations.  Token, score and flags equal the unconstrained
    kernel's on the masked logits at the same (seed, stream id, column): the mask enters before temperature, top-k and top-p and the
    draw's counter and stream are unchanged."""
    seen, m = run_sampled(get_backend(be_name), kind, V, ldl, 5, dev_pos, cols=MAX_LEN if V < 30000 else 4)
    if kind != "C2":
        assert seen["empty"] == 1, seen


@pytest.mark.parametrize("be_name", BACKENDS)
def test_sampled_selection_plain_and_prompted(be_name):
    """top-k and top-p off; then under a prompt: forced columns draw nothing and leave the state untouched"""
    be = get_backend(be_name)
    seen, _ = run_sampled(be, "single", 37, 40, 5, False, top_k=0, top_p=1.0)
    assert seen["finished"] > 0
    seen, _ = run_sampled(be, "single", 37, 40, 5, True, lens=[1, 3, 5, 2, 4])
    assert seen["forced"] == 0 + 2 + 4 + 1 + 3


# ---- validation ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("be_name", BACKENDS)
def test_constrained_entries_validate(be_name):
    """every MG_E_ARG case returns before it touches its outputs (sentinels), the accepted call at the end runs"""
    be = get_backend(be_name)
    lib = con_lib(be)
    rows, V, ldl = 2, 37, 40
    cls, table, _ = automaton("single", V)
    m = Run(be, rows, V, ldl, cls, table, [0, 1])
    lg = be.buf(padded(noise(rows, V, 1), ldl))
    o = Outs(be, rows, MAX_LEN, [1, 1], top2_cols=0)
    slot = be.zeros((64,), np.int32)

    def untouched():
        assert np.all(get(o.next) == SENT_ID) and np.all(get(o.out) == SENT_ID) and np.all(get(o.top2) == SENT32)
        assert np.array_equal(get(m.STATE), m.state) and int(get(m.EMPTY)[0]) == 0 and int(get(o.n_unf)[0]) == 0

    def con(**kw):
        c = MgkConstraint(m.CLS.ptr, m.TAB.ptr, table.shape[0], table.shape[1], m.STATE.ptr, m.EMPTY.ptr)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def greedy(c, **kw):
        d = SelDesc()
        d.logits, d.rows, d.V, d.ldl, d.eos, d.pad = lg.ptr, rows, V, ldl, EOS, PAD
        d.next_ids, d.out_ids, d.max_len, d.pos, d.min_len = o.next.ptr, o.out.ptr, MAX_LEN, 1, 0
        d.unfinished, d.n_unfinished, d.top2 = o.unf.ptr, o.n_unf.ptr, o.top2.ptr
        d.token_scores, d.ts_ld = o.ts.ptr, MAX_LEN - 1
        for k, v in kw.items():
            if k.startswith("slots_"):
                setattr(d.slots, k[6:], v)
            else:
                setattr(d, k, v)
        return lib.mgk_select_constrained(be.stream, C.byref(d), C.byref(c) if c is not None else None, None, None, 0, 0, None)

    def sampled(c, prompt=(None, None, 0, 0, None)):
        return lib.mgk_sample_select_constrained(be.stream, lg.ptr, rows, V, ldl, EOS, PAD, 0, 1.0, 0, 1.0, 5, None, o.next.ptr, o.out.ptr, MAX_LEN, 1,
                                                 None, o.unf.ptr, o.n_unf.ptr, None, o.ts.ptr, MAX_LEN - 1, o.top2.ptr,
                                                 C.byref(c) if c is not None else None, *prompt)

    bad = [None, con(cls=None), con(table=None), con(state=None), con(empty=None), con(n_classes=0), con(n_classes=4097), con(n_states=1),
           con(n_states=4097, n_classes=4096)]
    for call in (greedy, sampled):
        for c in bad:
            assert call(c) == MG_E_ARG
            untouched()
    assert greedy(con(), slots_pos=slot.ptr, slots_img=slot.ptr, slots_ctr=slot.ptr, slots_out_len=slot.ptr) == MG_E_ARG      # no queue form
    untouched()
    assert greedy(con(), ptop=slot.ptr) == MG_E_ARG and greedy(con(), fused=1, ptop=slot.ptr) == MG_E_ARG                      # no fused form
    untouched()
    assert sampled(con(), prompt=(slot.ptr, None, 1, 1, None)) == MG_E_ARG                                                     # a prompt without lengths
    untouched()
    assert greedy(con()) == 0
    assert np.all(get(o.next) != SENT_ID)
    assert sampled(con()) == 0


# ---- beam search -----------------------------------------------------------------------------------------------------------------------
# mgk_beam_step_constrained step by step against tests/constraint_script.beam_reference (pinned to stock in tests/test_constraint_stock.py):
# next ids, beam indices and the per-row states exactly - the states are those of the parents chosen, which checks the reordering - and
# scores within the 2e-5 that tests/test_beam_stock.py allows for float32 sums.
from markushgrapher_amd import constraint as K_                                  # noqa: E402
from markushgrapher_amd.constraint import TokenAutomaton                         # noqa: E402
from tests import constraint_script                                              # noqa: E402
from tests.beam_script import Script, tie_free                                   # noqa: E402
from tests.test_beam_kernels import EOS as BEOS, NAN_PAD, START, Logits, _lib as beam_lib, _read, _write, er_mid      # noqa: E402
from tests.test_decoder_prompt_kernels import beam_prompts                       # noqa: E402

BT_LIMIT = 1024 * 40          # BT_THREADS * BT_NPT: above it beam_row_topk_kernel streams the row instead of holding it in registers


def beam_con_lib(be):
    lib, P, I, F = beam_lib(be), C.c_void_p, C.c_int, C.c_float
    lib.mgk_beam_init_constrained.argtypes = [P, P, I, I, I, I, I, I, P, P, I, P, P, P, I, I, P, P, P]
    lib.mgk_beam_step_constrained.argtypes = [P, P, P, I, I, I, I, I, I, P, P, I, I, F, I, P, P, P, P, P, I, P]
    return lib


def beam_automaton(kind, V):
    """`bans`: banned tokens and words among the low ids the scripts like (every state allows nearly everything); `few`: state 0 allows
    three tokens only - fewer than 2K and no more than K - so -inf candidates are ranked and beams that take one move to the sink; then everything"""
    if kind == "bans":
        return K_.bad_words(V, BEOS, [[10, 11], [11, 12, 13], [14]]) & K_.suppress(V, BEOS, [0, 2, 5, 20, 21])
    Cn = min(V, 4000) + 1
    cls = np.minimum(np.arange(V), Cn - 1)
    table = np.full((3, Cn), -1, np.int64)
    table[0, [0, 2, 3]] = 1
    table[1, :] = 1
    table[1, BEOS] = table[2, BEOS] = 2
    return TokenAutomaton(cls, table, BEOS)


def run_beam_con(be, ref, aut, B, K, max_length, prompts, dev_pos, min_length=0, length_penalty=1.0, early_stopping=False, num_return=1, pad=0):
    lib = beam_con_lib(be)
    script = ref["script"]
    V, R = script.V, B * K
    ldl, T_cap = V + 14, max_length - 1
    lens = [len(p) for p in prompts]
    ld = max(lens) + 1
    pid = np.full((B, ld), V + 100, np.int64)
    for b, p in enumerate(prompts):
        pid[b, :len(p)] = p
    PID, LEN, BAD = be.buf(pid), be.buf(np.asarray(lens, np.int32)), be.buf(np.zeros(1, np.int32))
    CLS, TAB = be.buf(aut.cls), be.buf(aut.table)
    STATE, EMPTY, START_ST = be.buf(np.full(R, -9, np.int32)), be.buf(np.zeros(1, np.int32)), be.buf(np.asarray(ref["starts"], np.int32))
    con = MgkConstraint(CLS.ptr, TAB.ptr, aut.n_states, aut.n_classes, STATE.ptr, EMPTY.ptr)
    state = be.zeros(lib.mgk_beam_state_bytes(B, K, max_length), np.uint8)
    nid, bidx, ctr = be.zeros(R, np.int64), be.zeros(R, np.int32), be.zeros(8, np.int32)
    anc = be.zeros((T_cap, R), np.int32)
    div = be.buf(np.array([lib.mgk_beam_length_divisor(c, length_penalty) for c in range(max_length + 1)], np.float32))
    tdev = be.zeros(1, np.int32)
    lg = Logits(be, R, V, ldl, NAN_PAD)
    s = be.stream
    assert lib.mgk_beam_init_constrained(s, be.p(state), B, K, max_length, pad, BEOS, START, be.p(nid), be.p(anc), T_cap, be.p(ctr), be.p(PID),
                                         be.p(LEN), ld, V, be.p(BAD), C.byref(con), be.p(START_ST)) == 0
    assert np.array_equal(_read(be, STATE), np.repeat(ref["starts"], K))
    first = _read(be, nid)
    prefixes = [[int(first[r])] for r in range(R)]
    n_steps = 0
    for t in range(max_length - 1):
        lg.set({r: script.logits(r // K, prefixes[r]) for r in range(R)})
        if dev_pos:
            _write(be, tdev, np.array([t], np.int32))
        assert lib.mgk_beam_step_constrained(s, be.p(state), be.p(lg.dev), ldl, V, B, K, max_length, t + 1, be.p(tdev) if dev_pos else None,
                                             be.p(div), BEOS, min_length, C.c_float(length_penalty), int(early_stopping), be.p(nid), be.p(bidx),
                                             be.p(ctr), be.p(PID), be.p(LEN), ld, C.byref(con)) == 0
        n, bi, cont = _read(be, nid), _read(be, bidx), bool(_read(be, ctr)[0])
        n_steps += 1
        rs = ref["steps"][t]
        assert np.array_equal(n, rs["next_ids"]), ("next_ids", t, n, rs["next_ids"])
        assert np.array_equal(bi, rs["beam_idx"]), ("beam_idx", t, bi, rs["beam_idx"])
        assert cont == rs["cont"], ("continue flag", t)
        prefixes = [prefixes[bi[r]] + [int(n[r])] for r in range(R)]
        want = np.array([script.state(r // K, prefixes[r]) for r in range(R)])       # the automaton over what each row now holds
        assert np.array_equal(_read(be, STATE), want), ("states", t, _read(be, STATE), want)
        if not cont:
            break
    nr = num_return
    out_ids, out_cols, out_sc = be.zeros((B * nr, max_length), np.int64), be.zeros(1, np.int32), be.zeros(B * nr, np.float32)
    obi, ots = be.zeros((B * nr, max_length - 1), np.int32), be.zeros((B * nr, max_length - 1), np.float32)
    assert lib.mgk_beam_finalize(s, be.p(state), B, K, max_length, be.p(out_ids), be.p(out_cols), be.p(out_sc), nr, be.p(obi), be.p(ots)) == 0
    assert n_steps == len(ref["steps"]) and int(_read(be, EMPTY)[0]) == 0
    return dict(out_ids=_read(be, out_ids), scores=_read(be, out_sc), beam_indices=_read(be, obi), token_scores=_read(be, ots))


BEAM_CON = [
    # (kind, V, K, max_length, prompt lengths, options); B = 3
    ("bans", 500, 3, 12, [1, 4, 2], dict()),
    ("bans", 500, 5, 12, [1, 1, 1], dict(length_penalty=0.7, num_return=5, min_length=4)),
    ("few", 500, 3, 10, [1, 3, 1], dict(num_return=2)),
    ("few", 500, 5, 10, [2, 1, 4], dict(early_stopping=True, length_penalty=0.7, num_return=3)),
    ("bans", BT_LIMIT + 40, 3, 6, [1, 2, 1], dict()),                                            # the streaming branch
    ("few", BT_LIMIT + 40, 5, 6, [1, 1, 2], dict(num_return=2)),
]


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("case", BEAM_CON, ids=lambda c: "%s-V%d-K%d-P%s-%s" % (c[0], c[1], c[2], "_".join(map(str, c[4])), "-".join("%s%s" % (k[:3], v) for k, v in c[5].items())))
def test_beam_against_restatement(be_name, case):
    kind, V, K, ml, lens, o = case
    be = get_backend(be_name)
    B = 3
    aut = beam_automaton(kind, V)
    prompts = beam_prompts(lens, V)
    _, ref = tie_free(lambda seed: Script(V, BEOS, seed=seed, eos_rank=er_mid, n_hot=20),
                      lambda s: constraint_script.beam_reference(s, aut, B, K, ml, prompts, **o))
    nr = o.get("num_return", 1)
    seq = ref["sequences"]
    n = seq.shape[1] - 1
    finite = ref["scores"] > -1.0e8                                # hypotheses that were really finished with a finite score
    a = run_beam_con(be, ref, aut, B, K, ml, prompts, False, **o)
    assert np.array_equal(a["out_ids"][finite, :1 + n], seq[finite])
    assert np.array_equal(a["beam_indices"][finite, :n], ref["beam_indices"][finite])
    np.testing.assert_allclose(a["token_scores"][finite, :n], ref["token_scores"][finite], rtol=0, atol=2e-5)
    np.testing.assert_allclose(a["scores"][finite], ref["scores"][finite], rtol=0, atol=2e-5)
    assert finite.reshape(B, nr)[:, 0].all()                       # every image has a finite best hypothesis
    b = run_beam_con(be, ref, aut, B, K, ml, prompts, True, **o)  # the device-counter form: the same bits
    for k in ("out_ids", "scores", "beam_indices", "token_scores"):
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


@pytest.mark.parametrize("be_name", BACKENDS)
def test_beam_entries_validate(be_name):
    """every MG_E_ARG case of the two beam entries returns before it touches next_ids, the beam indices or the states (sentinels)"""
    be = get_backend(be_name)
    lib = beam_con_lib(be)
    B, K, V, ml = 2, 3, 50, 6
    aut = beam_automaton("bans", V)
    CLS, TAB = be.buf(aut.cls), be.buf(aut.table)
    STATE, EMPTY, ST0 = be.buf(np.full(B * K, -9, np.int32)), be.buf(np.zeros(1, np.int32)), be.buf(np.zeros(B, np.int32))
    state = be.zeros(lib.mgk_beam_state_bytes(B, K, ml), np.uint8)
    nid, bidx, ctr = be.buf(np.full(B * K, SENT_ID, np.int64)), be.buf(np.full(B * K, -5, np.int32)), be.zeros(8, np.int32)
    anc, div, lg = be.zeros((ml - 1, B * K), np.int32), be.buf(np.ones(ml + 1, np.float32)), be.zeros((B * K, V + 14), np.float32)

    def con(**kw):
        c = MgkConstraint(CLS.ptr, TAB.ptr, aut.n_states, aut.n_classes, STATE.ptr, EMPTY.ptr)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def init(c, start=ST0, prompt=(None, None, 0)):
        return lib.mgk_beam_init_constrained(be.stream, be.p(state), B, K, ml, 0, BEOS, START, be.p(nid), be.p(anc), ml - 1, be.p(ctr), *prompt, V,
                                             None, C.byref(c) if c is not None else None, be.p(start) if start is not None else None)

    def step(c, prompt=(None, None, 0), d=div):
        return lib.mgk_beam_step_constrained(be.stream, be.p(state), be.p(lg), V + 14, V, B, K, ml, 1, None, be.p(d) if d is not None else None,
                                             BEOS, 0, C.c_float(1.0), 0, be.p(nid), be.p(bidx), be.p(ctr), *prompt,
                                             C.byref(c) if c is not None else None)

    def untouched():
        assert np.all(_read(be, nid) == SENT_ID) and np.all(_read(be, bidx) == -5) and np.all(_read(be, STATE) == -9)

    bad = [None, con(cls=None), con(table=None), con(state=None), con(empty=None), con(n_classes=0), con(n_classes=4097), con(n_states=1),
           con(n_states=4097, n_classes=4096)]
    for c in bad:
        assert init(c) == MG_E_ARG and step(c) == MG_E_ARG
        untouched()
    assert init(con(), start=None) == MG_E_ARG and step(con(), d=None) == MG_E_ARG
    assert init(con(), prompt=(CLS.ptr, None, 1)) == MG_E_ARG and step(con(), prompt=(CLS.ptr, None, 1)) == MG_E_ARG      # a prompt without lengths
    untouched()
    assert init(con()) == 0 and np.all(_read(be, STATE) == 0) and step(con()) == 0
    assert np.all(_read(be, nid) != SENT_ID)
