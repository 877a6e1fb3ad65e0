"""Probe: scoring given target sequences at the benchmark's large shape (B = 32, recipe weights), T = 64 / 256 / 512, in ONE process:
   (a) the logits path: Engine.forward_logits + torch log_softmax, gather, argmax on the [B, T, vocab] fp32 logits
   (b) Engine.score: the lm_head with the log-softmax / argmax / gather in its epilogue (csrc/k_score.hip), no logits
and the lm_head stage alone on M = B * T rows: mgk_gemm (fp32 store) + the same torch ops against mgk_score.
   python tools/score_probe.py [--repeats 7] [--warmup 2] [--out profiles/score_probe.txt]
HIP events around each call, median of the repeats; torch.cuda.max_memory_allocated per path (reset before it; the engine's workspace is
allocated before either is measured, so the figures differ by what a path allocates per call)."""
import argparse, ctypes as C, os, statistics, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--lengths", type=int, nargs="+", default=[64, 256, 512])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from markushgrapher_amd import synth
    from markushgrapher_amd.engine import Engine
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    shape = synth.SHAPES["large"]
    sd = synth.recipe_state_dict(shape, **synth.BENCH_RECIPE)
    eng = Engine(shape, max_decode_len=512)
    eng.load_state_dict(sd)
    B, V, d = args.batch, shape.vocab_size, shape.d_model
    inp = synth.synth_batch(shape, B, seed=synth.BENCH_SEED, L_min=40, L_max=120)
    dt = {"input_ids": np.int64, "bbox": np.float32, "attention_mask": np.uint8, "pixel_values": np.float32}
    a = tuple(eng.mem.asarray(inp[k], dt[k]) for k in dt)
    dev = a[0].device
    say("large shape (vocab %d, d_model %d), B = %d, recipe weights; %s; median of %d after %d warm-up calls"
        % (V, d, B, torch.cuda.get_device_name(dev), args.repeats, args.warmup))

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        ms = []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return r, statistics.median(ms), min(ms), max(ms), torch.cuda.max_memory_allocated(dev)

    def torch_tail(logits, tg):
        lp = torch.log_softmax(logits, -1)
        return lp.gather(-1, tg[..., None])[..., 0], logits.argmax(-1)

    L = eng.lib
    L.mgk_score_scratch_bytes.restype = C.c_size_t
    L.mgk_score_scratch_bytes.argtypes = [C.c_int, C.c_int]
    L.mgk_score.argtypes = [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_void_p] * 6 + [C.c_size_t]
    L.mgk_gemm.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    P = lambda t: C.c_void_p(t.data_ptr())
    rng = np.random.default_rng(5)
    Vp = (V + 31) // 32 * 32
    def operand(rows, scale):
        """a packed bf16 operand of `rows` x d elements (rows a multiple of 32); for timing any finite bits do"""
        t = torch.from_numpy((rng.standard_normal(rows * d) * scale).astype(np.float32)).to(dev).to(torch.bfloat16).view(torch.int16)
        assert t.numel() == rows * d and rows % 32 == 0
        return t

    Wpk = operand(Vp, 0.05)
    for T in args.lengths:
        dec = torch.from_numpy(rng.integers(2, V, (B, T))).to(dev)
        tg = torch.from_numpy(rng.integers(2, V, (B, T))).to(dev)
        eng.score(*a, dec, tg)                       # grow the workspace once, before either path is measured
        torch.cuda.synchronize(dev)
        base = torch.cuda.memory_allocated(dev)

        def path_a():
            logits, _, _ = eng.forward_logits(*a, dec)
            return torch_tail(logits, tg)

        (lp_a, am_a), ta, ta0, ta1, ma = timed(path_a)
        (tok, arg, alp), tb, tb0, tb1, mb = timed(lambda: eng.score(*a, dec, tg))
        say("T = %3d  whole call  (a) forward_logits + torch log_softmax/gather/argmax: %8.3f ms [%.3f .. %.3f], peak +%8.1f MB"
            % (T, ta, ta0, ta1, (ma - base) / 1e6))
        say("                     (b) score():                                        %8.3f ms [%.3f .. %.3f], peak +%8.1f MB   (a)/(b) = %.2f x"
            % (tb, tb0, tb1, (mb - base) / 1e6, ta / tb))
        say("                     logits [B, T, vocab] fp32 = %.1f MB;  max |token log-prob (a) - (b)| = %.2e, argmax ids equal at %.4f of the positions"
            % (B * T * V * 4 / 1e6, float((lp_a - tok).abs().max()), float((am_a == arg).float().mean())))
        # the lm_head stage alone
        M = B * T
        Xpk = operand((M + 31) // 32 * 32, 1.0)
        flat_tg = tg.reshape(-1)
        nb = int(L.mgk_score_scratch_bytes(M, V))
        scratch = torch.empty(nb, dtype=torch.uint8, device=dev)
        o_tok, o_arg, o_alp = torch.empty(M, device=dev), torch.empty(M, dtype=torch.int64, device=dev), torch.empty(M, device=dev)
        st = eng.mem.stream()

        def head_a():
            logits = torch.empty((M, V), device=dev)
            assert L.mgk_gemm(st, 0, 0, P(Xpk), P(Wpk), M, V, d, P(logits), V, None, None) == 0
            return torch_tail(logits, flat_tg)

        def head_b():
            assert L.mgk_score(st, P(Xpk), P(Wpk), M, V, d, P(flat_tg), P(o_tok), P(o_arg), P(o_alp), None, P(scratch), nb) == 0

        _, ha, _, _, _ = timed(head_a)
        _, hb, _, _, _ = timed(head_b)
        say("         lm_head only, M = %5d: GEMM + torch ops %8.3f ms | fused %8.3f ms (%.1f TFLOP/s, partials %.1f MB)   ratio %.2f x"
            % (M, ha, hb, 2.0 * M * V * d / hb / 1e9, nb / 1e6, ha / hb))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
