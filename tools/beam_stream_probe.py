"""Probe: the cross-attention launches of ONE beam-5 decode layer at the bench geometry (d_model 1024, 16 heads, 32 images x 5 beams = 160
rows), through the C ABI hooks, in a fixed order so that a profiler's per-dispatch records can be matched to the configurations:

  kv           the K / V form (attn_step_kernel, group 5: the 5 rows of an image in one workgroup per head)
  row          the absorbed per-row stream (xattn_stream_kernel: one workgroup per row and split, no sharing between beams)
  beams        the absorbed beam stream (xattn_beams_kernel: BP beams of an image per workgroup) for the listed BP / ring / splits

Image lengths are drawn once (seed 0) around the bench's mean of ~1 050 attended positions per image; the script prints them and the
bytes of the states the launches must read at least (sum of attended positions x 2 d).  Timing and bytes come from the profiler:
  rocprofv3 --kernel-trace --stats -d <dir> --output-format csv -- python tools/beam_stream_probe.py --nt 1
  rocprofv3 --pmc FETCH_SIZE -d <dir> --output-format csv -- python tools/beam_stream_probe.py --nt 1 --reps 1
then  python tools/beam_stream_probe.py --parse <dir> [--reps N]  groups the dispatches by configuration (in launch order).
--d 768 --heads 12: the same at the widest geometry where three beams per workgroup exist."""
import argparse, csv, glob, json, os, sys
import ctypes as C
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")


def configs(d):
    cf = [("kv", 0, 0, 0), ("row", 0, 4, 1), ("row", 0, 4, 2)]
    cf += [("beams", 2, 4, s) for s in (1, 2, 3, 4)]
    cf += [("beams", 2, 3, s) for s in (1, 2)]
    if d <= 768:
        cf += [("beams", 3, 3, s) for s in (1, 2)]
    return cf


KERNELS = ("attn_step_kernel", "xattn_stream_kernel", "xattn_beams_kernel")


def parse(dirname, reps, d):
    cf = configs(d)
    tr = glob.glob(os.path.join(dirname, "**", "*kernel_trace.csv"), recursive=True)
    pm = glob.glob(os.path.join(dirname, "**", "*counter_collection.csv"), recursive=True)
    meta = json.load(open(os.path.join(dirname, "probe_meta.json"))) if os.path.exists(os.path.join(dirname, "probe_meta.json")) else {}
    if tr:
        rows = []
        for f in tr:
            for r in csv.DictReader(open(f)):
                if any(k in r["Kernel_Name"] for k in KERNELS):
                    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
        rows.sort()
        assert len(rows) == len(cf) * reps, (len(rows), len(cf), reps)
        for i, c in enumerate(cf):
            blk = rows[i * reps:(i + 1) * reps][1:]          # (first launch of a configuration: warm-up)
            us = np.array([(e - s) / 1e3 for s, e, _ in blk])
            print("%-6s BP %d ring %d splits %d  %-28s  median %7.1f us  min %7.1f" % (c[0], c[1], c[2], c[3], blk[0][2].split("(")[0][-28:],
                                                                                   np.median(us), us.min()))
    if pm:
        vals = []
        for f in pm:
            for r in csv.DictReader(open(f)):
                if any(k in r["Kernel_Name"] for k in KERNELS) and r["Counter_Name"] == "FETCH_SIZE":
                    vals.append((int(r.get("Dispatch_Id", 0)), float(r["Counter_Value"]), r["Kernel_Name"]))
        vals.sort()
        assert len(vals) == len(cf) * reps, (len(vals), len(cf), reps)
        need = meta.get("state_bytes")
        for i, c in enumerate(cf):
            kb = vals[i * reps][1]
            print("%-6s BP %d ring %d splits %d  FETCH_SIZE %9.0f KB = %7.1f MB%s" % (c[0], c[1], c[2], c[3], kb, kb * 1024 / 1e6,
                  "  (%.2f x the states)" % (kb * 1024 / need) if need and c[0] != "kv" else ""))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nt", type=int, default=1, help="1: the stream's copies non-temporal (engine default), 0: default policy")
    ap.add_argument("--reps", type=int, default=11, help="launches per configuration (the first is warm-up)")
    ap.add_argument("--d", type=int, default=1024)
    ap.add_argument("--heads", type=int, default=16)
    ap.add_argument("--parse", default=None, help="group a profiler output directory's dispatches by configuration")
    ap.add_argument("--meta-dir", default=None, help="write the state bytes here (probe_meta.json) for --parse")
    args = ap.parse_args()
    if args.parse:
        return parse(args.parse, args.reps, args.d)
    import torch
    from markushgrapher_amd import _lib
    lib = _lib.load()
    d, H, B, G = args.d, args.heads, 32, 5
    rows, inner = B * G, H * 64
    rs = np.random.RandomState(0)
    lens = rs.randint(960, 1141, size=B).astype(np.int32)
    cap = int((lens.max() + 63) // 64 * 64)
    state_bytes = int(lens.sum()) * 2 * d
    print("d %d, heads %d, %d images x %d beams, attended positions per image %d..%d (sum %d), states %.1f MB, nt %d"
          % (d, H, B, G, lens.min(), lens.max(), lens.sum(), state_bytes / 1e6, args.nt), flush=True)
    if args.meta_dir:
        os.makedirs(args.meta_dir, exist_ok=True)
        json.dump({"state_bytes": state_bytes, "lens": lens.tolist()}, open(os.path.join(args.meta_dir, "probe_meta.json"), "w"))
    dev = torch.device("cuda")

    gen = torch.Generator().manual_seed(0)
    bf = lambda n, s: (torch.randn(n, generator=gen) * s).to(torch.bfloat16).to(dev)
    q = bf(rows * H * 64, 0.5)
    wkv = torch.from_numpy((rs.standard_normal((2 * inner, d)) / np.sqrt(d)).astype(np.float32)).to(dev)
    enc = bf(B * cap * d, 1.0)
    kc, vc = bf(B * H * cap * 64, 1.0), bf(B * H * cap * 64, 1.0)
    L = torch.from_numpy(lens).to(dev)
    kv_row = torch.from_numpy(np.repeat(np.arange(B, dtype=np.int32), G)).to(dev)
    ctx = torch.zeros(((rows + 31) // 32 * 32) * inner, dtype=torch.bfloat16, device=dev)
    wk, wv = torch.empty(H * d * 64, dtype=torch.bfloat16, device=dev), torch.empty(H * d * 64, dtype=torch.bfloat16, device=dev)
    qx = torch.empty(rows * H * d, dtype=torch.bfloat16, device=dev)
    part = torch.empty(rows * 4 * H * d, dtype=torch.bfloat16, device=dev)
    ml = torch.empty(rows * 4 * H * 2, dtype=torch.float32, device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None
    if args.nt == 0:
        os.environ["MG_XATTN_NT"] = "0"        # (mgk_xattn reads the engine's switch)
    for kind, bp, nstg, ns in configs(d):
        for _ in range(args.reps):
            if kind == "kv":
                rc = lib.mgk_attention_step(st, P(q), P(kc), P(vc), P(ctx), rows, H, G, cap, P(L), 0, None, None, 0)
            elif kind == "row":
                rc = lib.mgk_xattn(st, P(q), P(wkv), P(enc), P(L), P(kv_row), rows, H, d, cap, ns, nstg, P(wk), P(wv), P(qx), P(part), P(ml), P(ctx))
            else:
                rc = lib.mgk_xattn_beams(st, P(q), P(wkv), P(enc), P(L), None, None, rows, H, d, cap, G, ns, nstg, bp, args.nt,
                                         P(wk), P(wv), P(qx), P(part), P(ml), P(ctx))
            assert rc == 0, (kind, bp, nstg, ns, rc)
        torch.cuda.synchronize()
    print("done: %d configurations x %d launches" % (len(configs(d)), args.reps), flush=True)


if __name__ == "__main__":
    main()
