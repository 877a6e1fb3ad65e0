"""Probe: the sampled queue (mg_generate_stream_sampled) beside the greedy queue and beside batch-form sampling, at the benchmark's large
shape with EOS live, max_length 512, one context, the same images everywhere:
   greedy queue, 32 slots | sampled queue S = 1, 32 slots | sampled queue S = 5, 255 slots (51 image-equivalents) |
   batch form generate_sampled(num_return = 5) in calls of 32 images (160 rows each)
   python tools/sampling_queue_probe.py [--queue 4] [--temperature 1.0] [--top-k 50] [--top-p 1.0] [--samples 5]
Rates are images/s (an image = all of its samples) and sequences/s; the queue's rows are checked against the batch form's."""
import argparse, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queue", type=int, default=4, help="batches of 32 images in the queue")
    ap.add_argument("--eos-scale", type=float, default=12.0)
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--top-k", type=int, default=50)
    ap.add_argument("--top-p", type=float, default=1.0)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args()
    import torch
    from markushgrapher_amd import synth
    from markushgrapher_amd.engine import Engine
    shape = synth.SHAPES["large"]
    sd = synth.recipe_state_dict(shape, **synth.BENCH_RECIPE)
    emb = sd["shared.weight"].copy()
    emb[shape.eos_token_id] = synth.round_bf16(sd["shared.weight"][shape.eos_token_id] * np.float32(args.eos_scale))
    sd["shared.weight"] = emb
    eng = Engine(shape, max_decode_len=512)
    eng.load_state_dict(sd)
    eng.set_stream_encoder(0)
    B, Q, S, T = 32, args.queue, args.samples, 512
    N = B * Q
    inp = synth.synth_batch(shape, N, seed=synth.BENCH_SEED, L_min=40, L_max=120)      # N different images
    dt = {"input_ids": np.int64, "bbox": np.float32, "attention_mask": np.uint8, "pixel_values": np.float32}
    dev = {k: eng.mem.asarray(inp[k], dt[k]) for k in dt}
    a = (dev["input_ids"], dev["bbox"], dev["attention_mask"], dev["pixel_values"])
    skw = dict(temperature=args.temperature, top_k=args.top_k, top_p=args.top_p, seed=args.seed)
    print("large shape, %d images, EOS live (scale %.0f), max_length %d; sampling: temperature %.2f top_k %d top_p %.2f"
          % (N, args.eos_scale, T, args.temperature, args.top_k, args.top_p), flush=True)

    def timed(fn):
        fn()
        torch.cuda.synchronize(); t0 = time.time()
        r = fn()
        torch.cuda.synchronize()
        return r, time.time() - t0

    (o, l, steps), tg = timed(lambda: eng.generate_stream(*a, max_length=T, chunk=B, slots=32, pool_chunks=3))
    lg = l.cpu().numpy()
    print("greedy queue, 32 slots:            %7.1f ms = %6.2f images/s, %d steps, %.2f ms per step, mean length %.1f"
          % (tg * 1e3, N / tg, steps, tg * 1e3 / steps, lg.mean()), flush=True)
    (o1, l1, steps1), t1 = timed(lambda: eng.generate_stream_sampled(*a, max_length=T, chunk=B, slots=32, pool_chunks=3, **skw))
    l1n = l1.cpu().numpy()
    print("sampled queue S = 1, 32 slots:     %7.1f ms = %6.2f images/s (%.2f x the greedy queue), %d steps, %.2f ms per step, mean length %.1f"
          % (t1 * 1e3, N / t1, tg / t1, steps1, t1 * 1e3 / steps1, l1n.mean()), flush=True)
    slots = min(255, 51 * S)
    (o5, l5, steps5), t5 = timed(lambda: eng.generate_stream_sampled(*a, max_length=T, num_return=S, chunk=B, slots=slots, pool_chunks=3, **skw))
    o5n, l5n = o5.cpu().numpy(), l5.cpu().numpy()
    print("sampled queue S = %d, %d slots:   %7.1f ms = %6.2f images/s = %7.2f sequences/s, %d steps, %.2f ms per step, mean length %.1f (min %d, max %d)"
          % (S, slots, t5 * 1e3, N / t5, N * S / t5, steps5, t5 * 1e3 / steps5, l5n.mean(), l5n.min(), l5n.max()), flush=True)

    # batch form: calls of 32 images x S samples, each waiting for its longest row; the same random streams as the queue's sequences
    def batch_calls():
        rows, cols = [], []
        for c0 in range(0, N, B):
            ids, n, _ = eng.generate_sampled(*(x[c0:c0 + B] for x in a), max_length=T, num_return=S, stream_ids=np.arange(c0 * S, (c0 + B) * S), **skw)
            rows.append(ids.cpu().numpy()); cols.append(n)
        return rows, cols
    eng.generate_sampled(*(x[:B] for x in a), max_length=T, num_return=S, **skw)      # workspace, capture
    torch.cuda.synchronize(); t0 = time.time()
    rows, cols = batch_calls()
    torch.cuda.synchronize(); tb = time.time() - t0
    nsteps = sum(c - 1 for c in cols)
    print("batch form, %d calls of 32 x %d:    %7.1f ms = %6.2f images/s = %7.2f sequences/s, %d steps of %d rows, %.2f ms per step"
          % (len(cols), S, tb * 1e3, N / tb, N * S / tb, nsteps, B * S, tb * 1e3 / nsteps), flush=True)
    print("sampled queue S = %d over the batch form: %.2f x" % (S, tb / t5), flush=True)
    # the queue's rows against the batch form's (same stream ids; both run the absorbed cross-attention at these row counts)
    same = 0
    for c, ids in enumerate(rows):
        for r in range(ids.shape[0]):
            q = c * B * S + r
            n = min(int(l5n[q]), ids.shape[1])
            same += bool(np.array_equal(o5n[q, :n], ids[r, :n]))
    print("rows of the S = %d queue equal to the batch form's: %d of %d" % (S, same, N * S), flush=True)


if __name__ == "__main__":
    main()
