"""Measurements of the sampling mode on one GPU (DESIGN.md section 4 "Sampled selection"; results under profiles/).

  python tools/sample_probe.py kernel     sample_select_kernel per launch beside greedy_select_kernel on the same fp32 logits
                                          (160 rows x 33 201, HIP events around 50 launches), filters off / top-k / top-p / both
  python tools/sample_probe.py calls      images/s of a 160-row call at the large shape (bench weights, 63 new tokens, EOS suppressed):
                                          greedy, sampled (top_k 50, top_p 0.95), sampled with 5 samples per image, beam-5
  MG_PROBE_LIB=<path>                     kernel mode: another build of the library (A/B of kernel forms)

Run `calls` under `rocprofv3 --kernel-trace --stats -- python tools/sample_probe.py calls sampled` for the kernel trace of one mode."""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def kernel():
    from markushgrapher_amd import _lib
    lib = C.CDLL(os.environ["MG_PROBE_LIB"]) if os.environ.get("MG_PROBE_LIB") else _lib.load()
    lib.mgk_sample_select.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int,
                                      C.c_float, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_int]
    rows, V, T = 160, 33201, 8
    ldl = (V + 31) // 32 * 32
    for sigma in (2.0, 6.0):
        lg = torch.randn(rows, ldl, device="cuda", generator=torch.Generator("cuda").manual_seed(1)) * sigma
        nxt = torch.zeros(rows, dtype=torch.int64, device="cuda")
        out = torch.zeros(rows, T, dtype=torch.int64, device="cuda")
        unf = torch.ones(rows, dtype=torch.int32, device="cuda")
        nu = torch.zeros(1, dtype=torch.int32, device="cuda")
        ts = torch.zeros(rows, T - 1, device="cuda")
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        p = lambda t: C.c_void_p(t.data_ptr())

        def timed(fn, n=50):
            for _ in range(5):
                unf.fill_(1)
                fn()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            tot = 0.0
            for _ in range(n):
                unf.fill_(1)
                a.record()
                fn()
                b.record()
                b.synchronize()
                tot += a.elapsed_time(b)
            return tot / n * 1e3

        g = timed(lambda: lib.mgk_greedy_select(st, p(lg), rows, V, ldl, -1, 0, 0, p(nxt), p(out), T, 1, p(unf), p(nu), None))
        print(f"sigma {sigma}: greedy_select (memset + kernel, event bracket) {g:7.1f} us", flush=True)
        for name, k, pp in (("filters off", 0, 1.0), ("top_k 50", 50, 1.0), ("top_p 0.95", 0, 0.95), ("top_k 50 + top_p 0.95", 50, 0.95)):
            s = timed(lambda: lib.mgk_sample_select(st, p(lg), rows, V, ldl, -1, 0, 0, 1.0, k, pp, 7, None, p(nxt), p(out), T, 1, p(unf),
                                                    p(nu), p(ts), T - 1))
            print(f"sigma {sigma}: sample_select {name:24s} {s:7.1f} us   (row bytes read once: {rows * V * 4 / 1e6:.1f} MB)", flush=True)


def calls(only=None):
    from tests.test_bench_config import _setup
    g, shape, eng, args = _setup()
    big = tuple(torch.cat([a] * 5, 0) if isinstance(a, torch.Tensor) else np.concatenate([a] * 5, 0) for a in args)
    T = 64

    def rate(name, images, fn, n=3):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / n
        print(f"{name:44s} {images / dt:8.1f} images/s  ({dt * 1e3:7.1f} ms per call, {images} images, 160 decode rows, 63 new tokens)", flush=True)

    modes = {
        "greedy": lambda: rate("greedy, 160 images", 160, lambda: eng.generate(*big, max_length=T, min_length=T)),
        "sampled": lambda: rate("sampled top_k 50 top_p 0.95, 160 images", 160,
                                lambda: eng.generate_sampled(*big, max_length=T, min_length=T, top_k=50, top_p=0.95, seed=1)),
        "sampled5": lambda: rate("sampled, 32 images x 5 samples", 32,
                                 lambda: eng.generate_sampled(*args, max_length=T, min_length=T, top_k=50, top_p=0.95, seed=1, num_return=5)),
        "beam5": lambda: rate("beam-5, 32 images", 32, lambda: eng.generate(*args, num_beams=5, max_length=T, min_length=T)),
    }
    for k, fn in modes.items():
        if only in (None, k):
            fn()


if __name__ == "__main__":
    if sys.argv[1] == "kernel":
        kernel()
    else:
        calls(sys.argv[2] if len(sys.argv) > 2 else None)
