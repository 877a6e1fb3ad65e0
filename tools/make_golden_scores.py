"""Mint tests/golden/scores_tiny.npz: token log-probabilities and the beam n-best list from STOCK transformers'
UdopForConditionalGeneration (transformers 5.15.0), the reference points of generate(return_dict_in_generate=True) and
compute_transition_scores on the HIP path (tests/test_scores.py).

Runs ONLY in the build container (as tools/make_golden.py, whose weights and inputs it reuses): G3 = the trained-tiny weights
(g3_weights.npz) on its 6 copy-task inputs, G0 = the recipe weights on the edge-case inputs.  Per fixture and case:
  greedy       sequences, compute_transition_scores(normalize_logits=True)
  greedy_min   the same with min_length = MIN_LEN (EOS suppressed in the normaliser while the sequence is shorter)
  beam         num_beams=5, num_return_sequences=5: sequences, sequences_scores, beam_indices, transition scores
  beam_es      the same with early_stopping=True and length_penalty=0.7
Full-vocab processed scores (output_scores) are stored for G0's 2 images only (size).

    python tools/make_golden_scores.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from markushgrapher_amd import synth  # noqa: E402
from tools.make_golden import G01_RECIPE, OUT, edge_case_inputs, versions  # noqa: E402
from tools.stock import stock_model  # noqa: E402
from tools.train_tiny import copy_task_batch  # noqa: E402

MAX_LEN, MIN_LEN, BEAMS = 16, 9, 5


def run(m, inp, prefix, full_scores):
    t = {k: torch.from_numpy(np.asarray(v)) for k, v in inp.items()}
    out = {}

    def gen(**kw):
        with torch.no_grad():
            return m.generate(input_ids=t["input_ids"], bbox=t["bbox"].clone(), pixel_values=t["pixel_values"],
                              attention_mask=t["attention_mask"], max_length=MAX_LEN, do_sample=False, return_dict_in_generate=True,
                              output_scores=True, **kw)
    for case, kw in (("greedy", dict(num_beams=1)), ("greedy_min", dict(num_beams=1, min_length=MIN_LEN))):
        g = gen(**kw)
        ts = m.compute_transition_scores(g.sequences, g.scores, normalize_logits=True)
        out[f"{prefix}.{case}.sequences"] = g.sequences.numpy()
        out[f"{prefix}.{case}.transition_scores"] = ts.numpy()
        if full_scores and case == "greedy":
            out[f"{prefix}.{case}.scores"] = torch.stack(g.scores, 1).numpy()
    for case, kw in (("beam", dict(num_beams=BEAMS, num_return_sequences=BEAMS)),
                     ("beam_es", dict(num_beams=BEAMS, num_return_sequences=BEAMS, early_stopping=True, length_penalty=0.7))):
        g = gen(**kw)
        ts = m.compute_transition_scores(g.sequences, g.scores, g.beam_indices, normalize_logits=False)
        out[f"{prefix}.{case}.sequences"] = g.sequences.numpy()
        out[f"{prefix}.{case}.sequences_scores"] = g.sequences_scores.numpy()
        out[f"{prefix}.{case}.beam_indices"] = g.beam_indices.numpy().astype(np.int32)
        out[f"{prefix}.{case}.transition_scores"] = ts.numpy()
        if full_scores and case == "beam":
            out[f"{prefix}.{case}.scores"] = torch.stack(g.scores, 1).numpy()
    return out


def main():
    shape = synth.SHAPES["tiny"]
    arrs = {}
    print("G3 trained tiny")
    sd3 = dict(np.load(os.path.join(OUT, "g3_weights.npz")))
    b = copy_task_batch(shape, 6, seed=99)
    b.pop("labels")
    arrs.update(run(stock_model(shape, sd3), b, "g3", False))
    print("G0 recipe weights / edge-case inputs")
    sd0 = synth.recipe_state_dict(shape, **G01_RECIPE)
    arrs.update(run(stock_model(shape, sd0), edge_case_inputs(shape), "g0", True))
    for k, v in arrs.items():
        print(f"   {k:34s} {tuple(v.shape)}")
    p = os.path.join(OUT, "scores_tiny.npz")
    np.savez_compressed(p, versions=versions(), max_length=np.int64(MAX_LEN), min_length=np.int64(MIN_LEN), num_beams=np.int64(BEAMS),
                        **arrs)
    print("   wrote", p, os.path.getsize(p), "bytes")


if __name__ == "__main__":
    main()
