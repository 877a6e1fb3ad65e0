"""Constrained decoding: token automata that the selection kernels consult and advance on the device (include/mgrapher.h,
mg_generate_constrained).

A TokenAutomaton is a finite automaton over token CLASSES.  Token t has class cls[t]; in state s it is allowed iff
table[s, cls[t]] >= 0, and that entry is the next state.  Two conventions hold for every automaton (the constructor checks them):
EOS is a class of its own, and the LAST state is the sink, which allows EOS only.  A row that emits a token its state does not allow
moves to the sink.

Everything here is numpy on the host: the builders compile the mask-type requests of generate() (banned tokens, banned words, tokens
banned at the first free position, "one of these sequences") to one table, `a & b` combines two, and allowed / step / run are the model
of what the device does, used by the tests.  The range checks of the table's entries live here, not in the C entry."""
import numpy as np

MAX_CLASSES = 4096
MAX_ENTRIES = 1 << 24


class TokenAutomaton:
    """cls [V], table [S, C], eos: see the module's header.  forced [S, C] (optional, host only) is the state after a token that was GIVEN,
    not chosen - a decoder prompt's: by default the table's entry, and the sink where the token is not allowed; the builders of history-free
    bans pass their own, since stock accepts a banned token inside a prompt (it only moves the state)."""

    def __init__(self, cls, table, eos, forced=None):
        cls = np.asarray(cls)
        table = np.asarray(table)
        if cls.ndim != 1 or cls.size < 1 or not np.issubdtype(cls.dtype, np.integer):
            raise ValueError("cls must be a non-empty 1-d integer array (the class of every token)")
        if table.ndim != 2 or not np.issubdtype(table.dtype, np.integer):
            raise ValueError("table must be a 2-d integer array [states, classes]")
        S, C = table.shape
        if C < 1 or C > MAX_CLASSES:
            raise ValueError("the automaton has %d classes; 1 .. %d are supported" % (C, MAX_CLASSES))
        if S < 2:
            raise ValueError("the automaton needs at least 2 states (the last one is the sink)")
        if S * C > MAX_ENTRIES:
            raise ValueError("a table of %d x %d entries exceeds 2**24" % (S, C))
        if cls.min() < 0 or cls.max() >= C:
            raise ValueError("cls holds a class outside [0, %d)" % C)
        if table.min() < -1 or table.max() >= S:
            raise ValueError("table holds an entry outside [-1, %d)" % S)
        eos = int(eos)
        if eos < 0 or eos >= cls.size:
            raise ValueError("eos (%d) outside [0, %d)" % (eos, cls.size))
        ce = int(cls[eos])
        if int((cls == ce).sum()) != 1:
            raise ValueError("EOS must be a class of its own (class %d holds %d tokens)" % (ce, int((cls == ce).sum())))
        sink = table[S - 1]
        if sink[ce] < 0 or (np.delete(sink, ce) >= 0).any():
            raise ValueError("the last state is the sink: it must allow EOS and nothing else")
        inhabited = np.bincount(cls, minlength=C) > 0
        dead = np.nonzero(~((table >= 0) & inhabited[None, :]).any(axis=1))[0]
        if dead.size:
            raise ValueError("state %d allows no token (every class it allows is empty)" % int(dead[0]))
        self.cls = np.ascontiguousarray(cls, np.uint16)
        self.table = np.ascontiguousarray(table, np.int32)
        self.eos = eos
        if forced is None:
            forced = np.where(table >= 0, table, S - 1)
        forced = np.asarray(forced)
        if forced.shape != table.shape or forced.min() < 0 or forced.max() >= S:
            raise ValueError("forced must be [states, classes] with entries in [0, %d)" % S)
        self.forced = np.ascontiguousarray(forced, np.int32)

    @property
    def n_states(self):
        return self.table.shape[0]

    @property
    def n_classes(self):
        return self.table.shape[1]

    @property
    def vocab(self):
        return self.cls.size

    @property
    def sink(self):
        return self.table.shape[0] - 1

    def allowed(self, state):
        """the token ids allowed in `state`, ascending"""
        return np.nonzero(self.table[state][self.cls] >= 0)[0]

    def allowed_mask(self, state):
        return self.table[state][self.cls] >= 0

    def step(self, state, tok):
        """the state after emitting `tok` in `state`; a token that is not allowed leads to the sink"""
        n = int(self.table[state, self.cls[int(tok)]])
        return self.sink if n < 0 else n

    def run(self, state, toks):
        for t in toks:
            state = self.step(state, t)
        return state

    def run_forced(self, state, toks):
        """the state after the GIVEN tokens `toks` (a decoder prompt after its start token)"""
        for t in toks:
            state = int(self.forced[state, self.cls[int(t)]])
        return state

    def __and__(self, other):
        """the product automaton: a token is allowed iff both allow it.  Its classes are the common refinement of the two partitions, its
        states the pairs reachable from (0, 0) (state 0), and its last state the sink"""
        if not isinstance(other, TokenAutomaton):
            return NotImplemented
        return product([self, other])[0]

    def as_prefix_allowed_tokens_fn(self, starts=None, prompt_lens=None):
        """stock generate's prefix_allowed_tokens_fn(batch_id, input_ids) for this automaton: image b is in starts[b] (default 0) after the
        first prompt_lens[b] (default 1: the start token) decoder tokens; a sequence in the sink gets [eos]"""
        def fn(batch_id, input_ids):
            b = int(batch_id)
            ids = [int(t) for t in input_ids]
            s = self.run(0 if starts is None else int(starts[b]), ids[(1 if prompt_lens is None else int(prompt_lens[b])):])
            return [self.eos] if s == self.sink else [int(t) for t in self.allowed(s)]
        return fn


def product(automata, starts=()):
    """the product of one or more automata -> (automaton, [state of every tuple of `starts`]).  Its states are the tuples of component
    states reachable from (0, .., 0) (state 0) and from the tuples of `starts` - the components' states after a prompt, which the free
    transitions alone need not reach - by free and by forced transitions; a tuple of sinks is the sink, the last state.  Its forced table
    is the components': `(a & b).run_forced(0, prompt)` is the pair of `a.run_forced` and `b.run_forced`."""
    automata = list(automata)
    a0 = automata[0]
    if any(a.vocab != a0.vocab or a.eos != a0.eos for a in automata):
        raise ValueError("the automata differ in vocabulary size or EOS")
    key = np.zeros(a0.vocab, np.int64)
    for a in automata:
        key = np.unique(key * a.n_classes + a.cls, return_inverse=True)[1].reshape(-1)
    C = int(key.max()) + 1
    rep_tok = np.zeros(C, np.int64)
    rep_tok[key] = np.arange(a0.vocab)                            # one token of every class of the refinement
    comp_cls = [a.cls[rep_tok].astype(np.int64) for a in automata]
    sink = tuple(a.sink for a in automata)
    zero = tuple(0 for _ in automata)
    index, order, rows, frows = {}, [], [], []
    for s in [zero] + [tuple(int(x) for x in s) for s in starts]:
        if s != sink and s not in index:
            index[s] = len(order)
            order.append(s)
    i = 0
    while i < len(order):
        st = order[i]
        i += 1
        nxt = np.stack([a.table[s][cc] for a, s, cc in zip(automata, st, comp_cls)])      # [components, C]
        row = np.full(C, -1, np.int64)
        for c in np.nonzero((nxt >= 0).all(0))[0]:
            n = tuple(int(x) for x in nxt[:, c])
            if n == sink:
                row[c] = -2                                       # (the sink is numbered last, below)
                continue
            if n not in index:
                index[n] = len(order)
                order.append(n)
            row[c] = index[n]
        rows.append(row)
        # given tokens (a prompt's): every component follows its own forced table, so a product keeps what its components accept
        fnx = np.stack([a.forced[s][cc] for a, s, cc in zip(automata, st, comp_cls)])
        frow = np.full(C, -2, np.int64)
        for c in range(C):
            n = tuple(int(x) for x in fnx[:, c])
            if n == sink:
                continue
            if n not in index:
                index[n] = len(order)
                order.append(n)
            frow[c] = index[n]
        frows.append(frow)
    S = len(order) + 1
    table = np.full((S, C), -1, np.int64)
    table[:S - 1] = np.stack(rows)
    table[table == -2] = S - 1
    table[S - 1, key[a0.eos]] = S - 1
    index[sink] = S - 1
    forced = np.full((S, C), S - 1, np.int64)
    forced[:S - 1] = np.stack(frows)
    forced[forced == -2] = S - 1
    return TokenAutomaton(key, table, a0.eos, forced=forced), [index[tuple(int(x) for x in s)] for s in starts]


def _classes(V, eos, tokens):
    """class 0 = every other token, then one class per token of `tokens` (ascending), EOS always among them -> (cls, {token: class})"""
    toks = sorted(set(int(t) for t in tokens) | {int(eos)})
    if toks[0] < 0 or toks[-1] >= V:
        raise ValueError("token id outside [0, %d)" % V)
    cls = np.zeros(V, np.int64)
    of = {}
    for k, t in enumerate(toks):
        cls[t] = of[t] = k + 1
    return cls, of


def unconstrained(V, eos):
    cls, of = _classes(V, eos, [])
    return TokenAutomaton(cls, [[0, 1], [-1, 1]], eos)


def suppress(V, eos, tokens):
    """the tokens are never allowed (stock suppress_tokens): one state and the sink"""
    banned = set(int(t) for t in tokens)
    cls = np.zeros(V, np.int64)
    if min(banned, default=0) < 0 or max(banned, default=0) >= V:
        raise ValueError("token id outside [0, %d)" % V)
    cls[sorted(banned)] = 2
    cls[eos] = 1
    return TokenAutomaton(cls, [[0, -1 if int(eos) in banned else 1, -1], [-1, 1, -1]], eos, forced=[[0, 0, 0], [1, 1, 1]])


def begin_suppress(V, eos, tokens):
    """the tokens are not allowed at the first free position (stock begin_suppress_tokens): state 0 there, state 1 afterwards, the sink"""
    banned = set(int(t) for t in tokens)
    if min(banned, default=0) < 0 or max(banned, default=0) >= V:
        raise ValueError("token id outside [0, %d)" % V)
    cls = np.zeros(V, np.int64)
    cls[sorted(banned)] = 2
    cls[eos] = 1
    return TokenAutomaton(cls, [[1, -1 if int(eos) in banned else 2, -1], [1, 2, 1], [-1, 2, -1]], eos,
                          forced=[[1, 1, 1], [1, 1, 1], [2, 2, 2]])


def _trie(words):
    children, terminal = [{}], [False]
    for w in words:
        n = 0
        for t in w:
            t = int(t)
            if t not in children[n]:
                children[n][t] = len(children)
                children.append({})
                terminal.append(False)
            n = children[n][t]
        terminal[n] = True
    return children, terminal


def bad_words(V, eos, words):
    """no banned word may be completed (stock bad_words_ids): the Aho-Corasick automaton of the word list, with the states that hold a
    complete word removed.  Classes: the tokens that occur in the words, EOS, and "other"."""
    words = [[int(t) for t in w] for w in words]
    if any(len(w) == 0 for w in words):
        raise ValueError("a banned word is empty")
    cls, of = _classes(V, eos, [t for w in words for t in w])
    C = len(of) + 1
    children, terminal = _trie(words)
    N = len(children)
    # breadth-first: failure links, the complete goto function over classes, and the nodes at which some word ends
    delta = np.zeros((N, C), np.int64)                            # (class 0 and tokens that start no word: back to the root)
    bad = list(terminal)
    fail = [0] * N
    queue = []
    for t, n in children[0].items():
        delta[0, of[t]] = n
        queue.append(n)
    i = 0
    while i < len(queue):
        n = queue[i]
        i += 1
        bad[n] = bad[n] or bad[fail[n]]
        delta[n] = delta[fail[n]]
        for t, ch in children[n].items():
            fail[ch] = int(delta[fail[n], of[t]])
            delta[n, of[t]] = ch
            queue.append(ch)
    keep = [n for n in range(N) if not bad[n]]
    if 0 not in keep:
        raise ValueError("the banned words leave nothing")
    idx = {n: k for k, n in enumerate(keep)}
    S = len(keep) + 1
    table = np.full((S, C), -1, np.int64)
    for n in keep:
        for c in range(C):
            nxt = int(delta[n, c])
            if not bad[nxt]:
                table[idx[n], c] = S - 1 if c == of[int(eos)] else idx[nxt]
    table[S - 1, of[int(eos)]] = S - 1
    # a given token that completes a banned word: the longest suffix that is still a state (stock looks at the last tokens, whatever they are)
    forced = np.full((S, C), S - 1, np.int64)
    for n in keep:
        for c in range(C):
            nxt = int(delta[n, c])
            while bad[nxt]:
                nxt = fail[nxt]
            forced[idx[n], c] = idx[nxt]
    return TokenAutomaton(cls, table, eos, forced=forced)


def one_of(V, eos, sequences):
    """the answer is one of the candidate sequences, each followed by EOS: the trie of the candidates (a trailing EOS of a candidate is
    dropped; the start token is not part of a candidate)"""
    seqs = []
    for s in sequences:
        s = [int(t) for t in s]
        if s and s[-1] == int(eos):
            s = s[:-1]
        if int(eos) in s:
            raise ValueError("a candidate holds EOS before its end")
        seqs.append(s)
    if not seqs:
        raise ValueError("no candidate sequences")
    cls, of = _classes(V, eos, [t for s in seqs for t in s])
    C = len(of) + 1
    children, terminal = _trie(seqs)
    S = len(children) + 1
    table = np.full((S, C), -1, np.int64)
    for n, ch in enumerate(children):
        for t, m in ch.items():
            table[n, of[t]] = m
        if terminal[n]:
            table[n, of[int(eos)]] = S - 1
    table[S - 1, of[int(eos)]] = S - 1
    return TokenAutomaton(cls, table, eos)


def one_of_each(V, eos, lists):
    """one automaton for a queue of images with their own candidate lists -> (automaton, starts [N]): a trie per image, all in one table.
    From state starts[n] exactly the sequences lists[n][j] + [eos] are accepted (candidates as one_of takes them: a trailing EOS is
    dropped, the start token is not part of a candidate; an empty candidate is the answer [eos]).  Images whose candidate SETS are equal
    share a root.  Classes: "other", then one per distinct token of all lists and EOS, ascending; the last state is the sink.  One table
    has to hold every trie: beyond 2**24 entries or 4096 classes a ValueError says how many images (the first k) fit - split the queue
    there, nothing is split here."""
    eos = int(eos)
    sets = []
    for n, cands in enumerate(lists):
        seqs = set()
        for s in cands:
            s = [int(t) for t in s]
            if s and s[-1] == eos:
                s = s[:-1]
            if eos in s:
                raise ValueError("a candidate of image %d holds EOS before its end" % n)
            if s and (min(s) < 0 or max(s) >= V):
                raise ValueError("token id outside [0, %d)" % V)
            seqs.add(tuple(s))
        if not seqs:
            raise ValueError("image %d has no candidate sequences" % n)
        sets.append(frozenset(seqs))
    if not sets:
        raise ValueError("no images")
    if eos < 0 or eos >= V:
        raise ValueError("eos (%d) outside [0, %d)" % (eos, V))
    children, terminal, root_of, starts = [], [], {}, []
    tokens = {eos}
    for n, seqs in enumerate(sets):
        if seqs not in root_of:
            root = root_of[seqs] = len(children)
            children.append({})
            terminal.append(False)
            for s in sorted(seqs):
                m = root
                for t in s:
                    if t not in children[m]:
                        children[m][t] = len(children)
                        children.append({})
                        terminal.append(False)
                    m = children[m][t]
                terminal[m] = True
                tokens.update(s)
            C, S = len(tokens) + 1, len(children) + 1
            if C > MAX_CLASSES or S * C > MAX_ENTRIES:
                raise ValueError("the automaton of %d images would have %d states x %d classes (limits: 2**24 entries, %d classes); the first "
                                 "%d images fit" % (n + 1, S, C, MAX_CLASSES, n))
        starts.append(root_of[seqs])
    cls, of = _classes(V, eos, tokens)
    C, S = len(of) + 1, len(children) + 1
    table = np.full((S, C), -1, np.int64)
    for n, ch in enumerate(children):
        for t, m in ch.items():
            table[n, of[t]] = m
        if terminal[n]:
            table[n, of[eos]] = S - 1
    table[S - 1, of[eos]] = S - 1
    return TokenAutomaton(cls, table, eos), np.asarray(starts, np.int32)
