"""Constrained greedy search on scripted logits: a float64 restatement of stock transformers `generate(prefix_allowed_tokens_fn=...)`,
built the way tests/prompt_script.py is (Script and tie rules of tests/beam_script.py).  The automaton's mask is applied where stock's
PrefixConstrainedLogitsProcessor applies it, beside MinLength, on the raw logits of the step; a prompt's tokens only move the state
(TokenAutomaton.run_forced).  Beam search: `Constrained` wraps a Script so that its processed log-probabilities carry the automaton's mask
after the log-softmax over the raw logits (stock's order), which makes tests/prompt_script.reference on the wrapped script the restatement
of stock's constrained beam search; the state of a beam is the automaton run over what it holds after its prompt."""
import math

import numpy as np

from tests.beam_script import MARGIN, TIE, NearTie


class Constrained:
    """a Script under an automaton: image b starts in starts[b] after its prompt of plen[b] tokens"""

    def __init__(self, script, automaton, plen, starts):
        self.script, self.automaton, self.plen, self.starts = script, automaton, list(plen), list(starts)
        self.V, self.eos = script.V, script.eos

    def state(self, image, prefix):
        return self.automaton.run(int(self.starts[image]), [int(t) for t in prefix[self.plen[image]:]])

    def logits(self, image, prefix):
        return self.script.logits(image, prefix)

    def log_probs(self, image, prefix, no_eos):
        """as Script.log_probs, over the whole row: the best 48 finite candidates in the selection order and the 18 lowest -inf ones"""
        x = self.script.logits(image, prefix).astype(np.float64)
        mx = x.max()
        lp = (x - mx) - math.log(math.fsum(np.exp(x - mx).tolist()))
        if no_eos:
            lp[self.eos] = -np.inf
        lp[~self.automaton.allowed_mask(self.state(image, prefix))] = -np.inf
        fin = np.flatnonzero(np.isfinite(lp))
        fin = fin[np.lexsort((fin, -lp[fin]))][:48]
        toks = np.concatenate([fin, np.flatnonzero(~np.isfinite(lp))[:18]]).astype(np.int64)
        return toks, lp[toks]


def beam_reference(script, automaton, B, K, max_length, prompts, starts=None, **options):
    """tests/prompt_script.reference under the automaton -> its result dict plus `script` (the wrapped one) and `starts`"""
    from tests import prompt_script
    if starts is None:
        starts = [automaton.run_forced(0, p[1:]) for p in prompts]
    wrapped = Constrained(script, automaton, [len(p) for p in prompts], starts)
    ref = prompt_script.reference(wrapped, B, K, max_length, prompts, **options)
    return dict(ref, script=wrapped, starts=np.asarray(starts))


def greedy_reference(script, automaton, prompts, max_length, images=None, min_length=0, pad=0, starts=None):
    """-> dict(sequences [B][cols] padded with `pad` after a row's EOS, token_scores [B][cols - 1] float64 log-softmax of the PROCESSED
    (masked) logits at the emitted token, 0.0 in prompt columns and after EOS, states [B] the automaton's state of every row at its end,
    starts [B] the state at the first free column).  starts: given, or what the prompt leaves."""
    B = len(prompts)
    images = list(range(B)) if images is None else list(images)
    rows, scores, states, first = [], [], [], []
    for b in range(B):
        seq = [int(t) for t in prompts[b]]
        st = automaton.run_forced(0, seq[1:]) if starts is None else int(starts[b])
        first.append(st)
        sc = [0.0] * (len(seq) - 1)
        while len(seq) < max_length:
            x = script.logits(images[b], seq).astype(np.float64)
            x[~automaton.allowed_mask(st)] = -np.inf
            if len(seq) < min_length:
                x[script.eos] = -np.inf
            assert np.isfinite(x).any(), "the case leaves a row with an empty allowed set"
            order = np.argsort(-x, kind="stable")
            if TIE < x[order[0]] - x[order[1]] < MARGIN:
                raise NearTie("near-tie in a greedy step")
            tok = int(order[0])
            mx = x.max()
            sc.append(float(x[tok] - mx - np.log(np.exp(x - mx).sum())))
            seq.append(tok)
            st = automaton.step(st, tok)
            if tok == script.eos:
                break
        rows.append(seq)
        scores.append(sc)
        states.append(st)
    cols = max(len(r) for r in rows)
    out = np.full((B, cols), pad, np.int64)
    ts = np.zeros((B, cols - 1))
    for b in range(B):
        out[b, :len(rows[b])] = rows[b]
        ts[b, :len(scores[b])] = scores[b]
    return dict(sequences=out, token_scores=ts, states=np.array(states), starts=np.array(first))
