"""Probe: attribution maps of given sequences at the benchmark's large shape (B = 32, recipe weights, bench inputs), T = 256 / 512, in ONE
process:
   (s) Engine.score:      the teacher-forced pass without maps (exists before attribute() did)
   (a) Engine.attribute:  the same stack plus one map launch per decoder layer (csrc/k_attrib.hip) and the gather
   (k) the map kernel alone, one layer, on operands of the call's shape (mgk_xattn_map), and the gather
   (t) the straightforward alternative, one layer: torch ops on the same packed-operand VALUES - einsum over the head dimension, masked
       softmax, mean over heads, accumulated into the map - with its peak allocation.  A whole call of it = (s) + layers x (t).
   python tools/attribution_probe.py [--repeats 7] [--warmup 2] [--out profiles/attribution.txt]
HIP events around each call, median of the repeats; torch.cuda.max_memory_allocated per path (reset before it)."""
import argparse, ctypes as C, os, statistics, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--lengths", type=int, nargs="+", default=[256, 512])
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
    B, V, H, NL, P = args.batch, shape.vocab_size, shape.num_heads, shape.num_decoder_layers, shape.num_patches
    inp = synth.synth_batch(shape, B, seed=synth.BENCH_SEED, L_min=40, L_max=120)
    dt = {"input_ids": np.int64, "bbox": np.float32, "attention_mask": np.uint8, "pixel_values": np.float32}
    a = tuple(eng.mem.asarray(inp[k], dt[k]) for k in dt)
    dev = a[0].device
    Lt = int(a[0].shape[1])
    S = Lt + P
    S_cap = (S + 63) // 64 * 64
    say("large shape (d_model %d, %d heads, %d decoder layers), B = %d, L = %d, keys per image %d; recipe weights; %s; median of %d after %d warm-up calls"
        % (shape.d_model, H, NL, B, Lt, S, torch.cuda.get_device_name(dev), args.repeats, args.warmup))

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

    L = eng.lib
    L.mgk_xattn_map_scratch_bytes.restype = C.c_size_t
    L.mgk_xattn_map_scratch_bytes.argtypes = [C.c_int] * 3
    L.mgk_xattn_map.argtypes = [C.c_void_p] * 3 + [C.c_int] * 5 + [C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_size_t] + [C.c_int] * 4 + \
        [C.c_void_p] * 3
    Pp = lambda t: C.c_void_p(t.data_ptr())
    rng = np.random.default_rng(5)

    def pack_rows(x):
        """bf16 [B, H, S, 64] -> HF_PK_ROWS [B][H][S/32][4][2][32][8]"""
        b, h, s, _ = x.shape
        return x.view(b, h, s // 32, 32, 4, 2, 8).permute(0, 1, 2, 4, 5, 3, 6).contiguous()

    need, base_ws = C.c_size_t(), C.c_size_t()
    for T in args.lengths:
        dec = torch.from_numpy(rng.integers(2, V, (B, T))).to(dev)
        tg = torch.from_numpy(rng.integers(2, V, (B, T))).to(dev)
        eng.attribute(*a, dec)                       # grow the workspace once, before anything is measured
        eng.score(*a, dec, tg)
        torch.cuda.synchronize(dev)
        base = torch.cuda.memory_allocated(dev)
        _, ts, ts0, ts1, _ = timed(lambda: eng.score(*a, dec, tg))
        (amap, enc_mask), ta, ta0, ta1, ma = timed(lambda: eng.attribute(*a, dec))
        assert L.mg_attribute_workspace_bytes(eng.model, B, Lt, T, 0, C.byref(need)) == 0
        assert L.mg_workspace_bytes(eng.model, B, Lt, 1, 0, T, 0, C.byref(base_ws)) == 0
        sums = amap.double().sum(-1)
        say("T = %3d  (s) score():     %8.3f ms [%.3f .. %.3f]" % (T, ts, ts0, ts1))
        say("         (a) attribute(): %8.3f ms [%.3f .. %.3f]   overhead over (s) %+.3f ms = %+.1f %%, %.3f ms per layer by the difference"
            % (ta, ta0, ta1, ta - ts, 100.0 * (ta - ts) / ts, (ta - ts) / NL))
        say("             allocates: map [B, T, L + P] fp32 %.1f MB per call (peak +%.1f MB incl. enc_out), workspace +%.1f MB behind the teacher-forced layout;"
            "  row sums in [%.6f, %.6f]" % (amap.numel() * 4 / 1e6, (ma - base) / 1e6, (need.value - base_ws.value) / 1e6, float(sums.min()), float(sums.max())))
        # one layer alone: kernel against torch ops on the same values
        T_cap = (T + 63) // 64 * 64
        q = (torch.randn(B, H, T_cap, 64, device=dev) * 0.5).to(torch.bfloat16)
        k = torch.randn(B, H, S_cap, 64, device=dev).to(torch.bfloat16)
        km = torch.zeros(B, S_cap, dtype=torch.uint8, device=dev)
        km[:, :S] = enc_mask
        qp, kp = pack_rows(q), pack_rows(k)
        nb = int(L.mgk_xattn_map_scratch_bytes(B, T, S))
        scratch = torch.empty(nb, dtype=torch.uint8, device=dev)
        out = torch.empty(B, T, S, device=dev)
        st = eng.mem.stream()

        def kern(acc, gather):
            assert L.mgk_xattn_map(st, Pp(qp), Pp(kp), B, H, T, T_cap, S_cap, Pp(km), acc, 1.0 / H if gather else 1.0, Pp(scratch), nb, 0, 0, S, 0,
                                   None, None, Pp(out) if gather else None) == 0

        kern(0, False)
        _, tk, tk0, tk1, _ = timed(lambda: kern(1, False))
        kern(0, False)
        _, tg_, _, _, _ = timed(lambda: kern(0, True))
        acc_t = torch.zeros(B, T, S, device=dev)

        def torch_layer():
            s = torch.einsum("bhqd,bhkd->bhqk", q[:, :, :T].float(), k[:, :, :S].float())
            s = s.masked_fill(km[:, None, None, :S] == 0, float("-inf"))
            acc_t.add_(torch.softmax(s, -1).mean(1))

        torch.cuda.synchronize(dev)
        base2 = torch.cuda.memory_allocated(dev)
        _, tt, tt0, tt1, mt = timed(torch_layer)
        acc_t.zero_()
        torch_layer()
        kern(0, True)
        err = float((out - acc_t).abs().max())
        say("         (k) map kernel, one layer (add form): %8.3f ms [%.3f .. %.3f] = %.1f TFLOP/s over two score passes; with the gather %8.3f ms; scratch %.1f MB"
            % (tk, tk0, tk1, 2 * 2.0 * B * H * T * S * 64 / tk / 1e9, tg_, nb / 1e6))
        say("         (t) torch ops, one layer:             %8.3f ms [%.3f .. %.3f], peak +%.1f MB;  max |kernel - torch| = %.2e;  (t)/(k) = %.1f x"
            % (tt, tt0, tt1, (mt - base2) / 1e6, err, tt / tk))
        say("             whole call the torch way = (s) + %d x (t) = %8.3f ms against (a) %8.3f ms: attribute() is %.2f x faster"
            % (NL, ts + NL * tt, ta, (ts + NL * tt) / ta))
        del q, k, qp, kp, scratch, out, acc_t
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
