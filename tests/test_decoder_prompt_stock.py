"""CPU: the float64 restatements of tests/prompt_script.py (greedy and beam search FROM A DECODER PROMPT) pinned to stock transformers
`generate` on the scripted model of tests/test_beam_stock.py, with `input_ids` as the prompt.  Equal-length prompts run as one stock batch;
ragged prompts as one stock call per image with its own prompt - the per-image semantics the device path implements.  Soft scripts take
their first tie-free seed, as that module does."""
import numpy as np
import pytest
import torch

from tests import prompt_script
from tests.beam_script import Script, tie_free

V, EOS, START = 500, 7, 1


def eos_schedule(image, cur_len):
    return 2 if (image + cur_len) % 3 == 0 else (6 if (image + cur_len) % 4 == 1 else None)


def stock_generate(script, images, prompts, K, max_length, min_length=0, length_penalty=1.0, early_stopping=False, num_return=1, pad=0):
    """one stock call on `images` (row r of the model = image images[r // K]) with the equal-length `prompts` as input_ids"""
    transformers = pytest.importorskip("transformers", reason="stock transformers is not installed")

    class Cfg(transformers.PretrainedConfig):
        model_type = "scripted_prompt"

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
    gc = transformers.GenerationConfig(num_beams=K, max_length=max_length, min_length=min_length, length_penalty=length_penalty,
                                       early_stopping=early_stopping, num_return_sequences=num_return, do_sample=False,
                                       eos_token_id=script.eos, pad_token_id=pad, bos_token_id=START, use_cache=False,
                                       return_dict_in_generate=True, output_scores=True)
    ids = torch.tensor(prompts, dtype=torch.long)
    with torch.no_grad():
        out = model.generate(input_ids=ids, generation_config=gc)
    if K > 1:
        ts = model.compute_transition_scores(out.sequences, out.scores, out.beam_indices, normalize_logits=False)
    else:
        ts = model.compute_transition_scores(out.sequences, out.scores, normalize_logits=True)
    return out, ts.numpy()


def prompts_of(lengths, seed=0):
    """prompt b: START, then tokens that are neither EOS nor the pad ids the cases use - except one forced EOS in the longest prompt"""
    r = np.random.RandomState(100 + seed)
    out = [[START] + [int(t) for t in r.choice(np.arange(10, V), n - 1, replace=False)] for n in lengths]
    b = int(np.argmax(lengths))
    if lengths[b] >= 3:
        out[b][lengths[b] - 2] = EOS                            # a forced EOS does not finish the row
    return out


# equal-length prompts in one batch: (lengths, K, max_length, options)
EQUAL = [
    ([1, 1], 3, 12, dict()),                                                                    # [start] alone: the unprompted call
    ([4, 4], 3, 12, dict()),
    ([3, 3, 3], 5, 20, dict(length_penalty=0.7, num_return=2)),
    ([5, 5], 5, 16, dict(length_penalty=0.0, num_return=5, pad=3)),
    ([4, 4], 5, 18, dict(early_stopping=True, min_length=8, num_return=5)),
    ([6, 6], 5, 14, dict(min_length=6)),                                                        # min_length = the first free column
    ([11, 11], 2, 12, dict()),                                                                  # one free column
]
# ragged prompts: one stock call per image
RAGGED = [
    ([1, 4], 3, 12, dict()),
    ([2, 7, 4], 5, 20, dict(length_penalty=0.7, num_return=5)),
    ([5, 1], 5, 16, dict(length_penalty=0.0, early_stopping=True, num_return=2)),
    ([3, 6], 5, 18, dict(min_length=7, num_return=5, pad=3)),
]


def _id(c):
    return "P%s-K%d-ml%d-%s" % ("_".join(map(str, c[0])), c[1], c[2], "-".join("%s%s" % (k[:3], v) for k, v in c[3].items()))


def _beam_ref(lengths, K, ml, o):
    prompts = prompts_of(lengths)
    script, ref = tie_free(lambda seed: Script(V, EOS, seed=seed, eos_rank=eos_schedule),
                           lambda s: prompt_script.reference(s, len(lengths), K, ml, prompts, **o))
    return prompts, script, ref


@pytest.mark.parametrize("case", EQUAL, ids=_id)
def test_beam_reference_matches_stock_batch(case):
    lengths, K, ml, o = case
    prompts, script, ref = _beam_ref(lengths, K, ml, o)
    B, P = len(lengths), lengths[0]
    out, ts = stock_generate(script, list(range(B)), prompts, K, ml, **o)
    assert np.array_equal(out.sequences.numpy(), ref["sequences"])
    # stock keeps no beam index / score for the prompt columns; the restatement holds the image's beam-0 row / 0.0 there
    assert np.array_equal(out.beam_indices.numpy(), ref["beam_indices"][:, P - 1:])
    nr = o.get("num_return", 1)
    assert np.array_equal(ref["beam_indices"][:, :P - 1], np.repeat(np.arange(B) * K, nr)[:, None].repeat(P - 1, 1))
    assert (ref["token_scores"][:, :P - 1] == 0).all()
    np.testing.assert_allclose(out.sequences_scores.numpy(), ref["scores"], rtol=0, atol=2e-5)
    np.testing.assert_allclose(ts, ref["token_scores"][:, P - 1:], rtol=0, atol=2e-5)


@pytest.mark.parametrize("case", RAGGED, ids=_id)
def test_beam_reference_matches_stock_per_image(case):
    lengths, K, ml, o = case
    prompts, script, ref = _beam_ref(lengths, K, ml, o)
    nr = o.get("num_return", 1)
    fill = o.get("pad", 0) or EOS
    for b, P in enumerate(lengths):
        out, ts = stock_generate(script, [b], [prompts[b]], K, ml, **o)
        seq, bi = out.sequences.numpy(), out.beam_indices.numpy()
        rows = slice(b * nr, (b + 1) * nr)
        n = bi.shape[1]                                         # generated columns of the image's longest hypothesis
        assert np.array_equal(ref["sequences"][rows, :P + n], seq), b
        assert (ref["sequences"][rows, P + n:] == fill).all()
        rbi = ref["beam_indices"][rows]
        assert np.array_equal(np.where(rbi[:, P - 1:P - 1 + n] < 0, -1, rbi[:, P - 1:P - 1 + n] - b * K), bi), b
        assert (rbi[:, :P - 1] == b * K).all() and (rbi[:, P - 1 + n:] == -1).all()
        np.testing.assert_allclose(out.sequences_scores.numpy(), ref["scores"][rows], rtol=0, atol=2e-5)
        np.testing.assert_allclose(ts, ref["token_scores"][rows, P - 1:P - 1 + n], rtol=0, atol=2e-5)
        assert (ref["token_scores"][rows, :P - 1] == 0).all()


GREEDY = [([1, 1, 1], 12, dict()), ([4, 4], 12, dict()), ([3, 3, 3], 20, dict(min_length=9)), ([1, 4, 7], 14, dict()),
          ([2, 6], 16, dict(min_length=8, pad=3))]


@pytest.mark.parametrize("case", GREEDY, ids=lambda c: "P%s-ml%d-%s" % ("_".join(map(str, c[0])), c[1], "-".join(c[2])))
def test_greedy_reference_matches_stock(case):
    lengths, ml, o = case
    prompts = prompts_of(lengths, seed=1)
    script, ref = tie_free(lambda seed: Script(V, EOS, seed=seed, eos_rank=eos_schedule),
                           lambda s: prompt_script.greedy_reference(s, prompts, ml, **o))
    B = len(lengths)
    groups = [list(range(B))] if len(set(lengths)) == 1 else [[b] for b in range(B)]
    pad = o.get("pad", 0)
    for g in groups:
        out, ts = stock_generate(script, g, [prompts[b] for b in g], 1, ml, **o)
        seq = out.sequences.numpy()
        P = lengths[g[0]]
        want = ref["sequences"][g]
        assert np.array_equal(want[:, :seq.shape[1]], seq) and (want[:, seq.shape[1]:] == pad).all(), g
        wts = ref["token_scores"][g][:, P - 1:seq.shape[1] - 1]
        live = np.cumsum(np.concatenate([np.zeros((len(g), 1), bool), seq[:, P:-1] == EOS], 1), 1) == 0      # stock scores the pad after EOS
        np.testing.assert_allclose(np.where(live, ts, 0.0), wts, rtol=0, atol=2e-5)
        assert (ref["token_scores"][g][:, :P - 1] == 0).all()
