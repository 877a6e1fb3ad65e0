"""Probe: what constrained decoding costs at the benchmark's large shape (B = 32, recipe weights, 256 forced columns), in ONE process:
   (a) whole calls, interleaved: greedy without a constraint (fused tail) against greedy under constraint.unconstrained() (unfused
       tail + class loads), and the same pair sampled and with beam-5;
   (b) the selection launch alone on 32 rows of the model's vocabulary: the plain scan / sampled selection against the constrained
       ones at C = 1 and C = 4096 classes (raw tables that allow everything).
   python tools/constraint_probe.py [--repeats 7] [--warmup 2] [--out profiles/constraint_probe.txt]
HIP events around each call (a) or around a run of launches (b), median of the repeats."""
import argparse, ctypes as C, os, statistics, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")


class SlotTab(C.Structure):      # include/mgrapher.h mgk_slot_table (unused here: the batch forms)
    _fields_ = [("pos", C.c_void_p), ("img", C.c_void_p), ("pool", C.c_void_p), ("ctr", C.c_void_p), ("out_len", C.c_void_p),
                ("pool_cap", C.c_int), ("start_id", C.c_int), ("first_tok", C.c_void_p), ("n_stop", C.c_int), ("stop", C.c_int * 4),
                ("max_len", C.c_int), ("nsamp", C.c_int)]


class SelDesc(C.Structure):      # include/mgrapher.h mgk_select_desc
    _fields_ = [("fused", C.c_int), ("logits", C.c_void_p), ("rows", C.c_int), ("V", C.c_int), ("ldl", C.c_int), ("eos", C.c_int),
                ("pad", C.c_int), ("suppress_eos", C.c_int), ("n_eos_more", C.c_int), ("eos_more", C.c_int * 3), ("next_ids", C.c_void_p),
                ("out_ids", C.c_void_p), ("max_len", C.c_int), ("pos", C.c_int), ("pos_dev", C.c_void_p), ("min_len", C.c_int),
                ("unfinished", C.c_void_p), ("n_unfinished", C.c_void_p), ("top2", C.c_void_p), ("step_ctr", C.c_void_p), ("slots", SlotTab),
                ("ptop", C.c_void_p), ("stopv", C.c_void_p), ("ntiles", C.c_int), ("tok_emb", C.c_void_p), ("h", C.c_void_p),
                ("gain", C.c_void_p), ("x_pk", C.c_void_p), ("x2_pk", C.c_void_p), ("x2_ld", C.c_int), ("x2_col0", C.c_int), ("d", C.c_int),
                ("eps", C.c_float), ("token_scores", C.c_void_p), ("ts_ld", C.c_int)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--columns", type=int, default=256)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from markushgrapher_amd import constraint as K, synth
    from markushgrapher_amd.engine import Engine, MgkConstraint
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    shape = synth.SHAPES["large"]
    sd = synth.recipe_state_dict(shape, **synth.BENCH_RECIPE)
    eng = Engine(shape, max_decode_len=512)
    eng.load_state_dict(sd)
    B, V, T = args.batch, shape.vocab_size, args.columns
    inp = synth.synth_batch(shape, B, seed=synth.BENCH_SEED, L_min=40, L_max=120)
    dt = {"input_ids": np.int64, "bbox": np.float32, "attention_mask": np.uint8, "pixel_values": np.float32}
    a = tuple(eng.mem.asarray(inp[k], dt[k]) for k in dt)
    dev = a[0].device
    say("large shape (vocab %d), B = %d, %d columns forced (min_length = max_length), recipe weights; %s; median of %d after %d warm-up calls"
        % (V, B, T, torch.cuda.get_device_name(dev), args.repeats, args.warmup))

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return r, e0.elapsed_time(e1)

    def pair(name, plain, con):
        """interleaved: plain, constrained, plain, ..."""
        for _ in range(args.warmup):
            plain(), con()
        tp, tc, rp, rc = [], [], None, None
        for _ in range(args.repeats):
            rp, t = once(plain)
            tp.append(t)
            rc, t = once(con)
            tc.append(t)
        mp, mc = statistics.median(tp), statistics.median(tc)
        say("%-8s whole call  plain %8.2f ms [%.2f .. %.2f] | unconstrained() %8.2f ms [%.2f .. %.2f]  difference %+.2f ms (%+.2f %%, %+.1f us per column)"
            % (name, mp, min(tp), max(tp), mc, min(tc), max(tc), mc - mp, 100.0 * (mc - mp) / mp, 1000.0 * (mc - mp) / (T - 1)))
        say("         ids identical: %s; captured step active: %s" % (bool(torch.equal(rp[0], rc[0])), bool(eng.decode_graph_active())))

    free = K.unconstrained(V, shape.eos_token_id)
    g = dict(max_length=T, min_length=T)
    pair("greedy", lambda: eng.generate(*a, **g), lambda: eng.generate(*a, constraint=free, **g))
    s = dict(max_length=T, min_length=T, temperature=1.0, top_k=50, top_p=0.95, seed=7)
    pair("sampled", lambda: eng.generate_sampled(*a, **s), lambda: eng.generate_sampled(*a, constraint=free, **s))
    bm = dict(num_beams=5, max_length=T, min_length=T)
    pair("beam-5", lambda: eng.generate(*a, **bm), lambda: eng.generate(*a, constraint=free, **bm))

    # (b) the selection launch alone
    L = eng.lib
    P, I, F = C.c_void_p, C.c_int, C.c_float
    L.mgk_select_ex.argtypes = [P, P]
    L.mgk_select_constrained.argtypes = [P, P, P, P, P, I, I, P]
    samp_args = [P, P, I, I, I, I, I, I, F, I, F, C.c_uint64, P, P, P, I, I, P, P, P, P, P, I]
    L.mgk_sample_select_constrained.argtypes = samp_args + [P, P, P, P, I, I, P]
    rows, ldl, max_len = B, (V + 31) // 32 * 32, 8
    rng = np.random.default_rng(3)
    lg = torch.from_numpy(rng.standard_normal((rows, ldl)).astype(np.float32)).to(dev)
    nxt, out = torch.zeros(rows, dtype=torch.int64, device=dev), torch.zeros((rows, max_len), dtype=torch.int64, device=dev)
    unf, n_unf = torch.ones(rows, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    ts = torch.zeros((rows, max_len - 1), device=dev)
    ptr = lambda t: t.data_ptr()
    st = eng.mem.stream()
    d = SelDesc()
    d.logits, d.rows, d.V, d.ldl, d.eos, d.pad = ptr(lg), rows, V, ldl, shape.eos_token_id, shape.pad_token_id
    for k in range(3):
        d.eos_more[k] = -1
    d.next_ids, d.out_ids, d.max_len, d.pos, d.min_len = ptr(nxt), ptr(out), max_len, 1, max_len
    d.unfinished, d.n_unfinished, d.token_scores, d.ts_ld = ptr(unf), ptr(n_unf), ptr(ts), max_len - 1

    def constraint(Cn):
        cls = torch.from_numpy((np.arange(ldl) % Cn).astype(np.int16)).to(dev)
        table = torch.zeros((2, Cn), dtype=torch.int32, device=dev)              # two states that allow everything and stay in state 0
        state, empty = torch.zeros(rows, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        return MgkConstraint(ptr(cls), ptr(table), 2, Cn, ptr(state), ptr(empty)), (cls, table, state, empty)

    def launches(fn):
        def run():
            for _ in range(args.launches):
                assert fn() == 0
        for _ in range(args.warmup):
            run()
        t = [once(run)[1] for _ in range(args.repeats)]
        return 1000.0 * statistics.median(t) / args.launches

    def sample(con):
        common = (st, ptr(lg), rows, V, ldl, shape.eos_token_id, shape.pad_token_id, max_len, 1.0, 50, 0.95, 7, None, ptr(nxt), ptr(out), max_len, 1,
                  None, ptr(unf), ptr(n_unf), None, ptr(ts), max_len - 1)
        return lambda: L.mgk_sample_select_constrained(*common, None, C.byref(con), None, None, 0, 0, None)

    c1, keep1 = constraint(1)
    c4096, keep2 = constraint(4096)
    say("selection launch alone, %d rows x %d logits, us per launch (%d launches back to back):" % (rows, V, args.launches))
    say("  greedy scan     plain %7.2f | C = 1 %7.2f | C = 4096 %7.2f"
        % (launches(lambda: L.mgk_select_ex(st, C.byref(d))),
           launches(lambda: L.mgk_select_constrained(st, C.byref(d), C.byref(c1), None, None, 0, 0, None)),
           launches(lambda: L.mgk_select_constrained(st, C.byref(d), C.byref(c4096), None, None, 0, 0, None))))
    L.mgk_sample_select.argtypes = [P, P, I, I, I, I, I, I, F, I, F, C.c_uint64, P, P, P, I, I, P, P, P, I]
    plain_s = lambda: L.mgk_sample_select(st, ptr(lg), rows, V, ldl, shape.eos_token_id, shape.pad_token_id, max_len, 1.0, 50, 0.95, 7, None,
                                          ptr(nxt), ptr(out), max_len, 1, ptr(unf), ptr(n_unf), ptr(ts), max_len - 1)
    say("  sampled         plain %7.2f | C = 1 %7.2f | C = 4096 %7.2f   (plain includes the entry's clear of the unfinished count)"
        % (launches(plain_s), launches(sample(c1)), launches(sample(c4096))))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
