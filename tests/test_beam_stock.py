"""CPU: the float64 beam-search reference of tests/beam_script.py pinned to stock transformers `generate` on scripted logits, and
oracle.udop_oracle.beam_search_core pinned to the same reference.  A minimal decoder-only model returns the script's row for each
row's prefix (image = row // num_beams); use_cache=False, decoder prompt [[start]].  Soft scripts take their first tie-free seed
(stock's torch.topk leaves the order of exact ties open)."""
import numpy as np
import pytest
import torch

from tests.beam_script import Script, reference, tie_free

V, EOS, START = 500, 7, 1


def eos_schedule(image, cur_len):
    return 2 if (image + cur_len) % 3 == 0 else (6 if (image + cur_len) % 4 == 1 else None)


def stock_generate(script, B, K, max_length, min_length=0, length_penalty=1.0, early_stopping=False, num_return=1, pad=0):
    transformers = pytest.importorskip("transformers", reason="stock transformers is not installed")

    class Cfg(transformers.PretrainedConfig):
        model_type = "scripted_beam"

    class Scripted(transformers.PreTrainedModel, transformers.GenerationMixin):
        config_class = Cfg

        def __init__(self, config):
            super().__init__(config)
            self.dummy = torch.nn.Parameter(torch.zeros(1))

        def forward(self, input_ids=None, **kw):
            rows = [script.logits(r // K, input_ids[r].tolist()) for r in range(input_ids.shape[0])]
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
    ids = torch.full((B, 1), START, dtype=torch.long)
    with torch.no_grad():
        out = model.generate(input_ids=ids, generation_config=gc)
    ts = model.compute_transition_scores(out.sequences, out.scores, out.beam_indices, normalize_logits=False)
    return out, ts.numpy()


# every option of the stock check: num_beams 2 / 5 / 8, length_penalty 1 / 0.7 / 0 / 2 / -0.5, early_stopping both, min_length 0 / middle /
# max_length, max_length 2 / short / 64, num_return 1 / 2 / K, pad 0 / nonzero
CASES = [
    dict(B=2, K=2, max_length=2),
    dict(B=3, K=5, max_length=20, length_penalty=0.7, num_return=2),
    dict(B=2, K=8, max_length=64, early_stopping=True),
    dict(B=3, K=5, max_length=30, min_length=10, length_penalty=-0.5),
    dict(B=2, K=5, max_length=8, min_length=8, length_penalty=2.0, num_return=5),
    dict(B=3, K=5, max_length=30, length_penalty=0.0, pad=3),
    dict(B=2, K=2, max_length=64, early_stopping=True, num_return=2, min_length=5),
    dict(B=2, K=8, max_length=16, length_penalty=0.7, num_return=8, pad=3, min_length=4),
]


def _ids(c):
    return "-".join("%s%s" % (k[:3], v) for k, v in c.items())


def _scripted(c):
    o = {k: v for k, v in c.items() if k not in ("B", "K", "max_length")}
    return tie_free(lambda seed: Script(V, EOS, seed=seed, eos_rank=eos_schedule),
                    lambda s: reference(s, c["B"], c["K"], c["max_length"], start=START, **o)), o


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_reference_matches_stock_generate(case):
    (script, ref), o = _scripted(case)
    out, ts = stock_generate(script, case["B"], case["K"], case["max_length"], **o)
    assert np.array_equal(out.sequences.numpy(), ref["sequences"])
    assert np.array_equal(out.beam_indices.numpy(), ref["beam_indices"])
    # float32 (stock) against float64: running sums of <= 64 log-probabilities of magnitude <= 60
    np.testing.assert_allclose(out.sequences_scores.numpy(), ref["scores"], rtol=0, atol=2e-5)
    np.testing.assert_allclose(ts, ref["token_scores"], rtol=0, atol=2e-5)


@pytest.mark.parametrize("case", [c for c in CASES if not c.get("min_length") and c.get("num_return", 1) == 1], ids=_ids)
def test_oracle_beam_search_core_matches_reference(case):
    from oracle.udop_oracle import beam_search_core
    c = dict(case, num_return=1)
    (script, ref), o = _scripted(c)
    B, K = c["B"], c["K"]

    def logits_fn(running_seq, cur_len):
        return torch.from_numpy(np.stack([script.logits(r // K, running_seq[r // K, r % K, :cur_len].tolist()) for r in range(B * K)]))

    ids, best = beam_search_core(logits_fn, lambda idx: None, B, K, V, c["max_length"], o.get("pad", 0), EOS, START,
                                 length_penalty=o.get("length_penalty", 1.0), early_stopping=o.get("early_stopping", False))
    assert np.array_equal(ids, ref["sequences"])
    np.testing.assert_allclose(best, ref["scores"], rtol=0, atol=2e-5)
