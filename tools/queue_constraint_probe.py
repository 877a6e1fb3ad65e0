"""Probe: what a decoder prompt / a constraint costs in the queue forms at the benchmark's large shape, in ONE process: a queue of 128
images (32 synthetic pages, four times), EOS enabled as bench.py enables it (the EOS row of the tied embedding scaled up bench.py's ladder
until three quarters of a 32-image batch end by themselves), max_length 512 -
   greedy queue on 32 slots and beam-5 queue on 32 image slots, each in three variants, interleaved:
   plain | constraint.unconstrained() | a prompt of [start] alone
   python tools/queue_constraint_probe.py [--repeats 5] [--warmup 1] [--images 128] [--out FILE]
Wall time around each call (the calls synchronise), median of the repeats; decode steps as the call reports them.  No threshold."""
import argparse, os, statistics, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")

EOS_ROW_SCALES = (3.0, 4.0, 6.0, 8.0, 12.0, 16.0)      # bench.py's ladder


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--images", type=int, default=128)
    ap.add_argument("--max-length", type=int, default=512)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from markushgrapher_amd import constraint as K, synth
    from markushgrapher_amd.engine import Engine
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    shape = synth.SHAPES["large"]
    sd = synth.recipe_state_dict(shape, **synth.BENCH_RECIPE)
    eng = Engine(shape, max_decode_len=512)
    eng.load_state_dict(sd)
    B, V, T, N = 32, shape.vocab_size, args.max_length, args.images
    inp = synth.synth_batch(shape, B, seed=synth.BENCH_SEED)
    dt = {"input_ids": np.int64, "bbox": np.float32, "attention_mask": np.uint8, "pixel_values": np.float32}
    a = tuple(eng.mem.asarray(inp[k], dt[k]) for k in dt)
    emb, chosen = sd["shared.weight"].copy(), None
    for scale in EOS_ROW_SCALES:
        emb[shape.eos_token_id] = synth.round_bf16(sd["shared.weight"][shape.eos_token_id] * np.float32(scale))
        eng.load_state_dict({"shared.weight": emb})
        ids = eng.generate(*a, max_length=T)[0].cpu().numpy()
        chosen = scale
        if (ids == shape.eos_token_id).any(axis=1).mean() >= 0.75:
            break
    reps = -(-N // B)
    q = tuple(torch.cat([x] * reps, dim=0)[:N].contiguous() for x in a)
    say("large shape (vocab %d), queue of %d images, max_length %d, EOS row scale %s, recipe weights; %s; median of %d after %d warm-up calls"
        % (V, N, T, chosen, torch.cuda.get_device_name(a[0].device), args.repeats, args.warmup))
    free = K.unconstrained(V, shape.eos_token_id)
    start = np.full((N, 1), shape.decoder_start_token_id, np.int64)
    variants = (("plain", {}), ("unconstrained()", dict(constraint=free)), ("[start] prompt", dict(decoder_prompt=start)))

    def family(name, call, kw):
        for _ in range(args.warmup):
            for _, v in variants:
                call(*q, **kw, **v)
        times = {n: [] for n, _ in variants}
        outs = {}
        for _ in range(args.repeats):
            for n, v in variants:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = call(*q, **kw, **v)
                torch.cuda.synchronize()
                times[n].append(time.perf_counter() - t0)
                outs[n] = r
        base = statistics.median(times["plain"])
        for n, _ in variants:
            m = statistics.median(times[n])
            r = outs[n]
            same = bool(torch.equal(r[0], outs["plain"][0]) and torch.equal(r[1], outs["plain"][1]))
            say("%-7s %-16s %8.1f ms [%.1f .. %.1f]  %7.1f images/s  steps %d  %+.2f %% against plain  ids and lengths equal plain: %s; captured step: %s"
                % (name, n, 1e3 * m, 1e3 * min(times[n]), 1e3 * max(times[n]), N / m, int(r[-1] if name == "beam-5" else r[2]),
                   100.0 * (m - base) / base, same, bool(eng.decode_graph_active())))

    family("greedy", eng.generate_stream, dict(max_length=T, chunk=B, slots=32, pool_chunks=3))
    family("beam-5", eng.generate_stream_beam, dict(num_beams=5, max_length=T, chunk=B, slots=32, pool_chunks=3))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
