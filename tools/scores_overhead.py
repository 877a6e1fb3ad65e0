"""Probe: decode step time with token scores on and off (include/mgrapher.h mg_gen_opts), at the benchmark's geometry.
   python tools/scores_overhead.py [--steps 64] [--reps 5] [--queue 64]
  greedy  one 160-row call (bench.py's 5 batches of 32 in one call; the weight-absorbed cross-attention, what such calls run), EOS
          suppressed for the whole length so every call runs the same steps: the lm_head epilogue adds the (max, sum) partials, the fused
          selection merges them
  beam    the beam-5 queue, 32 image slots, max_length 128 (mg_generate_stream_beam): the per-token log-probability history beside the beam-index
          history, the n-best copy-out of 5 hypotheses with scores and beam indices
Per leg: median over --reps calls of the call time / decode steps, scores off and on, alternated call by call."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64, help="greedy: decode steps per call (max_length - 1)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--queue", type=int, default=64, help="beam: images in the queue")
    args = ap.parse_args()
    import torch
    from markushgrapher_amd import synth
    from markushgrapher_amd.engine import Engine
    shape = synth.SHAPES["large"]
    eng = Engine(shape, max_decode_len=512)
    eng.load_state_dict(synth.recipe_state_dict(shape, **synth.BENCH_RECIPE))
    inp = synth.synth_batch(shape, 32, seed=synth.BENCH_SEED, return_pages=True)
    pix = eng.preprocess(inp["pages_u8"])
    cat = lambda a, n: torch.cat([torch.as_tensor(a).to(pix.device)] * n) if torch.is_tensor(a) or isinstance(a, np.ndarray) else a
    res = {}

    # greedy, 160 rows
    eng.set_cross_absorb(True)
    g = [cat(inp["input_ids"], 5), cat(inp["bbox"], 5), cat(inp["attention_mask"], 5), torch.cat([pix] * 5)]
    T = args.steps + 1
    times = {False: [], True: []}
    for r in range(args.reps + 1):
        for on in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = eng.generate(*g, max_length=T, min_length=T, return_scores=on)
            torch.cuda.synchronize()
            if r:                                      # the first round captures the graphs
                times[on].append((time.perf_counter() - t0) / args.steps * 1e3)
    off, on = float(np.median(times[False])), float(np.median(times[True]))
    res["greedy_160_rows_absorbed"] = {"step_ms_off": off, "step_ms_on": on, "overhead_pct": (on / off - 1) * 100,
                                       "off_all": times[False], "on_all": times[True]}

    # beam-5 queue, 32 slots
    n = args.queue
    reps = -(-n // 32)
    q = [cat(inp["input_ids"], reps)[:n], cat(inp["bbox"], reps)[:n], cat(inp["attention_mask"], reps)[:n], torch.cat([pix] * reps)[:n]]
    prev = eng.set_padding_semantics(True)
    times = {False: [], True: []}
    for r in range(args.reps + 1):
        for on in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = eng.generate_stream_beam(*q, num_beams=5, max_length=128, slots=32, chunk=32,
                                           num_return=5 if on else 1, return_scores=on)
            torch.cuda.synchronize()
            steps = out[3]
            if r:
                times[on].append((time.perf_counter() - t0) / steps * 1e3)
    eng.set_padding_semantics(prev)
    off, on = float(np.median(times[False])), float(np.median(times[True]))
    res["beam5_queue_32_slots"] = {"step_ms_off": off, "step_ms_on": on, "overhead_pct": (on / off - 1) * 100, "images": n,
                                   "off_all": times[False], "on_all": times[True]}
    for k, v in res.items():
        print(f"{k:28s} step {v['step_ms_off']:.4f} ms off, {v['step_ms_on']:.4f} ms on: {v['overhead_pct']:+.2f} %")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
