"""CPU: the float64 restatement of tests/constraint_script.py (greedy search under a token automaton) pinned to stock transformers
`generate(prefix_allowed_tokens_fn=automaton.as_prefix_allowed_tokens_fn(...))` on the scripted model of tests/test_beam_stock.py, with
and without a prompt; and the builders for suppress_tokens / begin_suppress_tokens / bad_words_ids pinned to stock's OWN processors for
those keywords through the same restatement.  Equal-length prompts run as one stock batch, ragged ones as one stock call per image.
Beam search (K = 3 and K = 5, with and without a prompt, min_length / length_penalty / early_stopping / num_return): the restatement is
tests/prompt_script.reference on the script wrapped by constraint_script.Constrained; only hypotheses with a finite score are compared (the
order among -inf ties is torch.topk's business), after asserting that every image keeps at least num_return of them."""
import numpy as np
import pytest
import torch

from markushgrapher_amd import constraint as K
from tests import constraint_script
from tests.beam_script import Script, tie_free
from tests.test_decoder_prompt_stock import EOS, START, V, eos_schedule, prompts_of


def stock_greedy(script, images, prompts, max_length, min_length=0, pad=0, K=1, **gen_kw):
    transformers = pytest.importorskip("transformers", reason="stock transformers is not installed")

    class Cfg(transformers.PretrainedConfig):
        model_type = "scripted_constraint"

    class Scripted(transformers.PreTrainedModel, transformers.GenerationMixin):
        config_class = Cfg

        def __init__(self, config):
            super().__init__(config)
            self.dummy = torch.nn.Parameter(torch.zeros(1))

        def forward(self, input_ids=None, **kw):
            rows = [script.logits(images[r // K], input_ids[r].tolist()) for r in range(input_ids.shape[0])]
            lg = torch.from_numpy(np.stack(rows))[:, None, :].expand(-1, input_ids.shape[1], -1)
            return transformers.modeling_outputs.CausalLMOutput(logits=lg)

        def prepare_inputs_for_generation(self, input_ids, **kw):
            return {"input_ids": input_ids}

    cfg = Cfg(vocab_size=script.V, eos_token_id=script.eos, pad_token_id=pad, bos_token_id=START)
    model = Scripted(cfg).eval()
    gc = transformers.GenerationConfig(num_beams=K, max_length=max_length, min_length=min_length, do_sample=False, eos_token_id=script.eos,
                                       pad_token_id=pad, bos_token_id=START, use_cache=False, return_dict_in_generate=True, output_scores=True,
                                       **{k: v for k, v in gen_kw.items() if k != "prefix_allowed_tokens_fn"})
    with torch.no_grad():
        out = model.generate(input_ids=torch.tensor(prompts, dtype=torch.long), generation_config=gc,
                             prefix_allowed_tokens_fn=gen_kw.get("prefix_allowed_tokens_fn"))
    if K > 1:
        return out, model.compute_transition_scores(out.sequences, out.scores, out.beam_indices, normalize_logits=False).numpy()
    return out, model.compute_transition_scores(out.sequences, out.scores, normalize_logits=True).numpy()


def plain_answers(lengths, ml, seed=1):
    """what the script writes unconstrained from these prompts: the material the automata are cut from"""
    from tests import prompt_script
    prompts = prompts_of(lengths, seed=seed)
    script, ref = tie_free(lambda s: Script(V, EOS, seed=s, eos_rank=eos_schedule), lambda s: prompt_script.greedy_reference(s, prompts, ml))
    return prompts, ref["sequences"]


def automata(prompts, plain):
    """automata that bite: they ban what the unconstrained rows write right after their prompts"""
    P = [len(p) for p in prompts]
    nxt = [int(plain[b, P[b]]) for b in range(len(prompts))]
    nx2 = [int(plain[b, P[b] + 1]) for b in range(len(prompts))]
    out = {
        "suppress": K.suppress(V, EOS, nxt),
        "bad_words": K.bad_words(V, EOS, [[nxt[0], nx2[0]], [nx2[-1]], [prompts[-1][-1], nxt[-1]] if P[-1] > 1 else [nxt[-1], nx2[-1]]]),
        "begin": K.begin_suppress(V, EOS, nxt + [EOS]),
        "few": K.one_of(V, EOS, [[nxt[0], 11, 12], [nxt[0], 13], [nx2[0]], [21, 22, 23, 24], [21, 25]]),      # states that allow 1 - 3 tokens
    }
    out["product"] = out["bad_words"] & out["begin"]
    return out


CASES = [([1, 1, 1], 12, dict()), ([4, 4], 12, dict()), ([3, 3, 3], 20, dict(min_length=9)), ([1, 4, 7], 14, dict()),
         ([2, 6], 16, dict(min_length=8, pad=3))]
NAMES = ["suppress", "bad_words", "begin", "few", "product"]


# Stock's token scores are a float32 log-softmax over V terms, the restatement's a float64 one of the same float32 logits.  A float32 sum
# of V positive terms carries a relative error of at most V * 2^-24 (sequential order, the worst case), which is the absolute error of its
# logarithm; the subtraction and the log add a few ulps of a value of order 1.  (The beam tests' 2e-5 is below this bound for V = 500 and
# was missed here by 6e-7 on one element.)
TS_ATOL = (V + 8) * 2.0 ** -24


def _groups(lengths):
    B = len(lengths)
    return [list(range(B))] if len(set(lengths)) == 1 else [[b] for b in range(B)]


def _compare(out, ts, ref, g, P, pad):
    seq = out.sequences.numpy()
    want = ref["sequences"][g]
    assert np.array_equal(want[:, :seq.shape[1]], seq) and (want[:, seq.shape[1]:] == pad).all(), (g, seq, want)
    wts = ref["token_scores"][g][:, P - 1:seq.shape[1] - 1]
    live = np.cumsum(np.concatenate([np.zeros((len(g), 1), bool), seq[:, P:-1] == EOS], 1), 1) == 0      # stock scores the pad after EOS
    np.testing.assert_allclose(np.where(live, ts, 0.0), wts, rtol=0, atol=TS_ATOL)


# (an answer of at most 3 tokens below min_length is the empty-set case, which stock does not have: "few" runs without min_length)
PAIRS = [(c, n) for c in CASES for n in NAMES if not (n == "few" and c[2].get("min_length", 0) > 0)]


@pytest.mark.parametrize("case,name", PAIRS, ids=lambda v: v if isinstance(v, str) else "P%s-ml%d-%s" % ("_".join(map(str, v[0])), v[1], "-".join(v[2])))
def test_greedy_reference_matches_stock_prefix_fn(case, name):
    lengths, ml, o = case
    prompts, plain = plain_answers(lengths, ml)
    aut = automata(prompts, plain)[name]
    # begin_suppress_tokens belongs to the first FREE column: its component starts after the prompt (modeling.py _constraint)
    starts = None
    if name in ("begin", "few"):
        starts = [0] * len(prompts)
    elif name == "product":
        bw = automata(prompts, plain)["bad_words"]
        aut, starts = K.product([bw, automata(prompts, plain)["begin"]], starts=[(bw.run_forced(0, p[1:]), 0) for p in prompts])
    script, ref = tie_free(lambda s: Script(V, EOS, seed=s, eos_rank=eos_schedule),
                           lambda s: constraint_script.greedy_reference(s, aut, prompts, ml, starts=starts, **o))
    assert not np.array_equal(ref["sequences"][:, :plain.shape[1]], plain[:, :ref["sequences"].shape[1]])     # the automaton bites
    for g in _groups(lengths):
        fn = aut.as_prefix_allowed_tokens_fn(starts=[ref["starts"][b] for b in g], prompt_lens=[lengths[b] for b in g])
        out, ts = stock_greedy(script, g, [prompts[b] for b in g], ml, prefix_allowed_tokens_fn=fn, **o)
        _compare(out, ts, ref, g, lengths[g[0]], o.get("pad", 0))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "P%s-ml%d-%s" % ("_".join(map(str, c[0])), c[1], "-".join(c[2])))
def test_builders_match_stocks_own_processors(case):
    """suppress_tokens, begin_suppress_tokens and bad_words_ids as stock's generate takes them, against the restatement under the builders'
    automata started the way model.generate starts them: run_forced over the prompt, begin_suppress at the first free column"""
    lengths, ml, o = case
    prompts, plain = plain_answers(lengths, ml)
    P = lengths
    nxt = [int(plain[b, P[b]]) for b in range(len(prompts))]
    nx2 = [int(plain[b, P[b] + 1]) for b in range(len(prompts))]
    words = [[nxt[0], nx2[0]], [nx2[-1]]] + ([[prompts[-1][-1], nxt[-1]]] if P[-1] > 1 else [])      # one word begins inside the last prompt
    sup = [nxt[1], prompts[0][-1]]                                                                     # one banned token sits in a prompt
    for kw, aut, follows in ((dict(suppress_tokens=sup), K.suppress(V, EOS, sup), True),
                             (dict(bad_words_ids=words), K.bad_words(V, EOS, words), True),
                             (dict(begin_suppress_tokens=nxt), K.begin_suppress(V, EOS, nxt), False)):
        starts = None if follows else [0] * len(prompts)
        script, ref = tie_free(lambda s: Script(V, EOS, seed=s, eos_rank=eos_schedule),
                               lambda s: constraint_script.greedy_reference(s, aut, prompts, ml, starts=starts, **o))
        for g in _groups(lengths):
            out, ts = stock_greedy(script, g, [prompts[b] for b in g], ml, **kw, **o)
            _compare(out, ts, ref, g, lengths[g[0]], o.get("pad", 0))


# ---- beam search -----------------------------------------------------------------------------------------------------------------------
def beam_automaton(kind):
    """`bans`: banned words and tokens among the low ids (the base tokens the scripts rank first); `few`: state 0 allows three tokens only (no more than K, so exact ties among them drop none),
    fewer than 2K for K = 3 and K = 5, so -inf candidates are really ranked; afterwards everything is allowed"""
    if kind == "bans":
        return K.bad_words(V, EOS, [[10, 11], [11, 12, 13], [14]]) & K.suppress(V, EOS, [0, 2, 5, 20, 21])
    table = np.full((3, V), -1, np.int64)
    table[0, [0, 2, 3]] = 1
    table[1, :] = 1
    table[1, EOS] = table[2, EOS] = 2
    return K.TokenAutomaton(np.arange(V), table, EOS)


BEAM = [
    # (kind, prompt lengths, K, max_length, options)
    ("bans", [1, 1], 3, 12, dict()),
    ("bans", [4, 4], 5, 20, dict(length_penalty=0.7, num_return=2, min_length=7)),
    ("bans", [1, 4, 2], 5, 20, dict(early_stopping=True, num_return=3)),
    ("few", [1, 1, 1], 3, 16, dict(num_return=2)),
    ("few", [3, 3], 5, 20, dict(length_penalty=0.7, num_return=3)),
    ("few", [2, 1, 4], 5, 20, dict(early_stopping=True, length_penalty=0.0, num_return=2, pad=3)),
]


@pytest.mark.parametrize("case", BEAM, ids=lambda c: "%s-P%s-K%d-%s" % (c[0], "_".join(map(str, c[1])), c[2], "-".join("%s%s" % (k[:3], v) for k, v in c[4].items())))
def test_beam_reference_matches_stock_prefix_fn(case):
    kind, lengths, Kb, ml, o = case
    aut = beam_automaton(kind)
    prompts = prompts_of(lengths)
    B, nr = len(lengths), o.get("num_return", 1)
    script, ref = tie_free(lambda s: Script(V, EOS, seed=s, eos_rank=eos_schedule),
                           lambda s: constraint_script.beam_reference(s, aut, B, Kb, ml, prompts, starts=[0] * B if kind == "few" else None, **o))
    finite = ref["scores"] > -1.0e8
    assert finite.reshape(B, nr).all()                             # first: every image keeps num_return finite finished hypotheses
    fill = o.get("pad", 0) or EOS
    for g in _groups(lengths):
        fn = aut.as_prefix_allowed_tokens_fn(starts=[ref["starts"][b] for b in g], prompt_lens=[lengths[b] for b in g])
        out, ts = stock_greedy(script, g, [prompts[b] for b in g], ml, K=Kb, prefix_allowed_tokens_fn=fn,
                               length_penalty=o.get("length_penalty", 1.0), early_stopping=o.get("early_stopping", False),
                               num_return_sequences=nr, min_length=o.get("min_length", 0), pad=o.get("pad", 0))
        rows = np.concatenate([np.arange(b * nr, (b + 1) * nr) for b in g])
        P = lengths[g[0]]
        seq = out.sequences.numpy()
        want = ref["sequences"][rows]
        m = min(seq.shape[1], want.shape[1])
        assert np.array_equal(want[:, :m], seq[:, :m]) and (want[:, m:] == fill).all() and (seq[:, m:] == fill).all(), (g, seq, want)
        np.testing.assert_allclose(out.sequences_scores.numpy(), ref["scores"][rows], rtol=0, atol=2e-5)
        n = min(ts.shape[1], ref["token_scores"].shape[1] - (P - 1))
        np.testing.assert_allclose(ts[:, :n], ref["token_scores"][rows, P - 1:P - 1 + n], rtol=0, atol=2e-5)
