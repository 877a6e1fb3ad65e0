"""Probe: the reference's default decode mode (beam-5, EOS live, max_length 512) as batch calls against the beam queue
(mg_generate_stream_beam), one context or several (--contexts 4: bench.py's beam5_eos_enabled_queue).
   python tools/beam_queue_probe.py [--slots 32] [--queue 8] [--contexts 4] [--beam-absorb [--beam-key-splits N]] [--forced]
--beam-absorb: beam search with the weight-absorbed cross-attention (Engine.set_beam_cross_absorb; default the K / V form).
--forced: also the 32-image, 128-token beam-5 batch alone and 4 in flight (bench.py's beam5 / beam5_in_flight)."""
import argparse, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, nargs="+", default=[32, 48])
    ap.add_argument("--queue", type=int, default=8, help="batches of 32 images in the queue")
    ap.add_argument("--eos-scale", type=float, default=12.0)
    ap.add_argument("--contexts", type=int, default=1, help="> 1: the queue on that many execution contexts at once (markushgrapher_amd/inflight.py), a queue of --queue batches each")
    ap.add_argument("--beam-absorb", action="store_true", help="beam search with the weight-absorbed cross-attention (mg_set_beam_cross_absorb)")
    ap.add_argument("--beam-key-splits", type=int, default=0, help="key splits of the absorbed beam stream (1..4; 0 = the library's default)")
    ap.add_argument("--forced", action="store_true", help="also the forced-length legs: 32 images x 128 tokens beam-5, alone and 4 in flight")
    ap.add_argument("--forced-only", action="store_true", help="only the forced-length legs (no EOS-live batch call or queue)")
    ap.add_argument("--tools-lib", action="store_true", help="the tools build of the library (MG_WHATIF_STEP what-if runs: wrong results, valid timing)")
    args = ap.parse_args()
    import torch
    from markushgrapher_amd import synth
    from markushgrapher_amd.engine import Engine
    shape = synth.SHAPES["large"]
    sd = synth.recipe_state_dict(shape, **synth.BENCH_RECIPE)
    emb = sd["shared.weight"].copy()
    emb[shape.eos_token_id] = synth.round_bf16(sd["shared.weight"][shape.eos_token_id] * np.float32(args.eos_scale))
    sd["shared.weight"] = emb
    if args.tools_lib:
        from tools import _toolslib
        eng = Engine(shape, lib=_toolslib.load(), max_decode_len=512)
    else:
        eng = Engine(shape, max_decode_len=512)
    eng.load_state_dict(sd)
    if args.beam_absorb:          # (before any clone: the contexts below inherit it)
        eng.set_beam_cross_absorb(True, args.beam_key_splits)
    print("beam cross-attention form: %s" % ("absorbed, key splits %s" % (args.beam_key_splits or "default") if eng.beam_cross_absorb else "K / V"), flush=True)
    B = 32
    inp = synth.synth_batch(shape, B, seed=synth.BENCH_SEED, return_pages=True)
    dt = {"input_ids": np.int64, "bbox": np.float32, "attention_mask": np.uint8, "pages_u8": np.uint8}
    dev = {k: eng.mem.asarray(inp[k], dt[k]) for k in dt}

    if args.forced_only:
        return forced(eng, dev, B)

    def batch():
        out, sc, _ = eng.generate(dev["input_ids"], dev["bbox"], dev["attention_mask"], eng.preprocess(dev["pages_u8"]), num_beams=5,
                                  max_length=512, min_length=0)
        return out.cpu().numpy(), sc.cpu().numpy()
    batch()
    torch.cuda.synchronize(); t0 = time.time()
    ref, ref_sc = batch()
    torch.cuda.synchronize(); tb = time.time() - t0
    print("batch call: %.1f ms per 32 images = %.2f images/s, %d columns" % (tb * 1e3, B / tb, ref.shape[1]), flush=True)
    if args.forced:
        forced(eng, dev, B)
    Q = args.queue
    q = {k: torch.cat([dev[k]] * Q, dim=0) for k in ("input_ids", "bbox", "attention_mask")}
    eng.set_stream_encoder(0)
    if args.contexts > 1:
        from markushgrapher_amd.inflight import InFlight
        fl = InFlight(eng, args.contexts)
        for c in fl.contexts:
            c.set_stream_encoder(0)
        for slots in args.slots:
            def job(ctx, i):
                pix = torch.cat([ctx.preprocess(dev["pages_u8"]) for _ in range(Q)], dim=0)
                o, l, sc, st = ctx.generate_stream_beam(q["input_ids"], q["bbox"], q["attention_mask"], pix, num_beams=5, max_length=512, min_length=0,
                                                        chunk=B, slots=slots, pool_chunks=3)
                return o.cpu().numpy(), l.cpu().numpy(), st
            fl.map(job, range(len(fl)))
            torch.cuda.synchronize(); t0 = time.time()
            res = fl.map(job, range(len(fl)))
            torch.cuda.synchronize(); tq = time.time() - t0
            same = all(np.array_equal(o[n, :min(int(l[n]), ref.shape[1])], ref[n % B, :min(int(l[n]), ref.shape[1])]) for o, l, _ in res for n in range(Q * B))
            print("queue on %d contexts, %d image slots each: %.2f images/s, steps %s, %.2f ms per step, hypotheses equal %s"
                  % (len(fl), slots, len(fl) * Q * B / tq, [int(r[2]) for r in res], tq * 1e3 / max(int(r[2]) for r in res), same), flush=True)
        fl.close()
        return
    for slots in args.slots:
        def queue():
            pix = torch.cat([eng.preprocess(dev["pages_u8"]) for _ in range(Q)], dim=0)
            return eng.generate_stream_beam(q["input_ids"], q["bbox"], q["attention_mask"], pix, num_beams=5, max_length=512, min_length=0,
                                            chunk=B, slots=slots, pool_chunks=3)
        queue()
        torch.cuda.synchronize(); t0 = time.time()
        o, l, sc, steps = queue()
        torch.cuda.synchronize(); tq = time.time() - t0
        o, l, sc = o.cpu().numpy(), l.cpu().numpy(), sc.cpu().numpy()
        same = all(np.array_equal(o[n, :min(int(l[n]), ref.shape[1])], ref[n % B, :min(int(l[n]), ref.shape[1])]) for n in range(Q * B))
        same_sc = bool(np.array_equal(sc, np.tile(ref_sc, Q)))
        print("queue, %d image slots: %.1f ms per 32 images = %.2f images/s (%.2f x), %d steps, %.2f ms per step, mean length %.1f, hypotheses equal %s, scores equal %s"
              % (slots, tq / Q * 1e3, Q * B / tq, (Q * B / tq) / (B / tb), steps, tq * 1e3 / steps, l.mean(), same, same_sc), flush=True)


def forced(eng, dev, B):
    """bench.py's beam5 / beam5_in_flight: 32 images, num_beams 5 (160 rows), 128 new tokens with EOS suppressed; alone, then 8 batches
    over 4 execution contexts."""
    import torch
    from markushgrapher_amd.inflight import InFlight

    def job(ctx):
        out, _, _ = ctx.generate(dev["input_ids"], dev["bbox"], dev["attention_mask"], ctx.preprocess(dev["pages_u8"]), num_beams=5,
                                 max_length=129, min_length=129)
        return out
    job(eng)
    torch.cuda.synchronize(); t0 = time.time()
    job(eng)
    torch.cuda.synchronize(); t1 = time.time() - t0
    print("forced beam5 (32 images, 128 tokens), alone: %.1f ms per batch = %.2f images/s" % (t1 * 1e3, B / t1), flush=True)
    fl = InFlight(eng, 4)
    for f in [fl.submit(job) for _ in range(len(fl))]:
        f.result()
    nb = 2 * len(fl)
    torch.cuda.synchronize(); t0 = time.time()
    for f in [fl.submit(job) for _ in range(nb)]:
        f.result()
    torch.cuda.synchronize(); t4 = time.time() - t0
    print("forced beam5 in flight (%d batches on %d contexts): %.1f ms per batch = %.2f images/s" % (nb, len(fl), t4 / nb * 1e3, B * nb / t4), flush=True)
    fl.close()


if __name__ == "__main__":
    main()
