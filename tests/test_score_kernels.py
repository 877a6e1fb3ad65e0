"""The fused lm_head scoring kernel (csrc/k_score.hip) through its test entry mgk_score: log-sum-exp, target log-probability, argmax and
its log-probability per row, without the [M][N] logits.

Reference: float64 numpy on the bf16-rounded inputs.  Tolerances: the kernel accumulates in fp32 on the matrix cores, so a logit is off by
at most K * 2^-24 * sum_k |x w| (computed per case below and asserted to stay under the figure the tolerance was derived from); a
log-probability is the difference of a logit and the log-sum-exp, each within that bound, plus the exp / log error of a few 1e-6 relative:
twice the bound with margin = 1e-3 at K = 128 (bound 2.7e-4) and 2e-3 at K = 192 (bound 5.9e-4).  The argmax must be exact wherever the
float64 top-2 gap exceeds twice the bound - asserted for every row of the random cases, so no row is excused."""
import ctypes as C

import numpy as np
import pytest

from tests import pkutil as pk
from tests.backends import get_backend

BACKENDS = [pytest.param("emu"), pytest.param("hip", marks=pytest.mark.gpu)]
SLAB = 1024          # the kernel's compile-time column partition (SC_SLAB)
SENT_F, SENT_I = np.float32(-77.25), np.int64(-777)


def bf16(x):
    """fp32 -> nearest-even bf16 -> fp32 (local restatement; finite inputs)"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint32) << 16
    return r.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def _inputs(M, N, K):
    x = bf16(np.random.default_rng(21).standard_normal((M, K)).astype(np.float32))
    w = bf16((np.random.default_rng(22).standard_normal((N, K)) * 0.3).astype(np.float32))
    tg = np.random.default_rng(23).integers(0, N, M).astype(np.int64)
    return x, w, tg


def _ref(x, w):
    lg = x.astype(np.float64) @ w.astype(np.float64).T
    mx = lg.max(1)
    lse = mx + np.log(np.exp(lg - mx[:, None]).sum(1))
    bound = x.shape[1] * 2.0 ** -24 * (np.abs(x).astype(np.float64) @ np.abs(w).astype(np.float64).T).max()
    top2 = np.sort(lg, 1)[:, -2:]
    return lg, lse, bound, (top2[:, 1] - top2[:, 0])


def _declare(lib):
    lib.mgk_score_scratch_bytes.restype = C.c_size_t
    lib.mgk_score_scratch_bytes.argtypes = [C.c_int, C.c_int]
    lib.mgk_score.argtypes = [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_void_p] * 6 + [C.c_size_t]


def _run(be, x, w, tg, M=None, skip=None, extra=7):
    """mgk_score on the first M rows; outputs are `extra` rows longer than M and pre-filled with sentinels.  skip: name of the output (or
    'targets') passed as a null pointer."""
    _declare(be.lib)
    M = x.shape[0] if M is None else M
    N, K = w.shape
    X, W = be.buf(pk.pack_tiles(x[:M])), be.buf(pk.pack_tiles(w))
    T = be.buf(tg[:M].astype(np.int64))
    o = {"tok_lp": be.buf(np.full(M + extra, SENT_F, np.float32)), "arg_id": be.buf(np.full(M + extra, SENT_I, np.int64)),
         "arg_lp": be.buf(np.full(M + extra, SENT_F, np.float32)), "lse": be.buf(np.full(M + extra, SENT_F, np.float32))}
    nb = int(be.lib.mgk_score_scratch_bytes(M, N))
    assert 0 < nb <= 256 + ((N + SLAB - 1) // SLAB) * ((M + 31) // 32 * 32) * 16          # a small multiple of M, never of M * N
    scratch = be.buf(np.full(nb // 4, 0x7FC00000, np.uint32))                              # (stale NaNs: nothing may be read before written)
    p = {k: (None if k == skip else v) for k, v in o.items()}
    rc = be.lib.mgk_score(be.stream, be.p(X), be.p(W), M, N, K, be.p(None if skip == "targets" else T), be.p(p["tok_lp"]),
                          be.p(p["arg_id"]), be.p(p["arg_lp"]), be.p(p["lse"]), be.p(scratch), nb)
    assert rc == 0
    res = {k: v.numpy().copy() for k, v in o.items()}
    res["err"] = int(scratch.numpy().view(np.int32)[0])
    for k, v in res.items():
        if k != "err":
            assert np.all(v[M:] == (SENT_I if k == "arg_id" else SENT_F)), f"{k}: rows >= M were written"
    return res


def _check(res, x, w, tg, tol, M=None):
    M = x.shape[0] if M is None else M
    lg, lse, bound, gap = _ref(x[:M], w)
    assert gap.min() > 2 * bound                     # every row's argmax is decided under the accumulation error
    assert np.array_equal(res["arg_id"][:M], lg.argmax(1))
    live = tg[:M] >= 0
    ref_tok = np.where(live, lg[np.arange(M), np.where(live, tg[:M], 0)] - lse, 0.0)
    for k, ref in (("lse", lse), ("arg_lp", lg.max(1) - lse), ("tok_lp", ref_tok)):
        err = np.abs(res[k][:M].astype(np.float64) - ref).max()
        print(f"{k}: max abs error {err:.3e} (bound {bound:.3e}, min gap {gap.min():.3e})")
        assert err < tol, k
    assert np.all(res["tok_lp"][:M][~live] == 0.0)
    assert res["err"] == 0
    return bound


@pytest.mark.parametrize("be_name", BACKENDS)
def test_random_parity(be_name):
    be = get_backend(be_name)
    x, w, tg = _inputs(70, 500, 128)
    bound = _check(_run(be, x, w, tg), x, w, tg, 1e-3)
    assert bound < 2.8e-4                            # the figure 1e-3 was derived from


@pytest.mark.parametrize("be_name", BACKENDS)
def test_all_negative_rows(be_name):
    """Every real logit of ten rows is below 0 = the logit of a pad column: a pad column that leaked in would be the argmax and would dominate
    the log-sum-exp."""
    be = get_backend(be_name)
    x, w, tg = _inputs(70, 500, 128)
    w = -np.abs(w)
    rows = np.arange(3, 70, 7)[:10]
    x[rows] = np.abs(x[rows])
    res = _run(be, x, w, tg)
    lg, lse, bound, _ = _ref(x, w)
    assert lg[rows].max() < 0
    assert np.all((res["arg_id"][:70] >= 0) & (res["arg_id"][:70] < 500))
    assert np.all(lg[np.arange(70), res["arg_id"][:70]] >= lg.max(1) - 2 * bound)
    for k, ref in (("lse", lse), ("arg_lp", lg.max(1) - lse), ("tok_lp", lg[np.arange(70), tg] - lse)):
        assert np.abs(res[k][:70] - ref).max() < 1e-3, k


@pytest.mark.parametrize("be_name", BACKENDS)
def test_exact_ties_take_the_lowest_index(be_name):
    """Bitwise duplicate columns: inside one 32-column tile, in the two half-waves' row groups of a tile, in the two column waves of a
    128-column step, in two steps of a slab, and in two slabs of the partition.  x = 4 w[n1] makes the duplicated column the row's maximum."""
    be = get_backend(be_name)
    x, w, tg = _inputs(70, 1100, 128)
    pairs = [(33, 50), (64, 69), (130, 200), (260, 700), (300, SLAB + 36)]
    for r, (n1, n2) in enumerate(pairs):
        w[n2] = w[n1]
        for rr in (r, 32 + r, 64 + r):               # rows of every 32-row tile of the call
            x[rr] = 4.0 * w[n1]
    res = _run(be, x, w, tg)
    lg = x.astype(np.float64) @ w.astype(np.float64).T
    for r, (n1, n2) in enumerate(pairs):
        for rr in (r, 32 + r, 64 + r):
            assert set(np.flatnonzero(lg[rr] == lg[rr].max())) == {n1, n2}
            assert res["arg_id"][rr] == n1, (rr, n1, n2, res["arg_id"][rr])


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("M,N", [(33, 481), (33, 512), (1, 500), (32, 500), (33, 500)])
def test_edge_shapes(be_name, M, N):
    be = get_backend(be_name)
    x, w, tg = _inputs(M, N, 128)
    tg[::3] = -100                                   # ignore_index
    full = _run(be, x, w, tg)                        # (rows >= M keep their sentinels: checked in _run)
    _check(full, x, w, tg, 1e-3)
    for skip in ("tok_lp", "arg_id", "arg_lp", "lse", "targets"):
        res = _run(be, x, w, tg, skip=skip)
        for k in ("tok_lp", "arg_id", "arg_lp", "lse"):
            if k == skip or (skip == "targets" and k == "tok_lp"):
                assert np.all(res[k] == (SENT_I if k == "arg_id" else SENT_F))      # a null output / no targets: nothing written
            else:
                assert np.array_equal(res[k].view(np.uint8), full[k].view(np.uint8)), (skip, k)


@pytest.mark.parametrize("be_name", BACKENDS)
def test_target_out_of_range_is_counted(be_name):
    be = get_backend(be_name)
    x, w, tg = _inputs(33, 500, 128)
    tg[4], tg[20] = 500, 40000
    res = _run(be, x, w, tg)
    assert res["err"] == 2 and res["tok_lp"][4] == 0.0 and res["tok_lp"][20] == 0.0


@pytest.mark.parametrize("be_name", BACKENDS)
def test_rows_do_not_depend_on_the_call(be_name):
    be = get_backend(be_name)
    x, w, tg = _inputs(70, 500, 128)
    a, a2, b = _run(be, x, w, tg), _run(be, x, w, tg), _run(be, x, w, tg, M=33)
    for k in ("tok_lp", "arg_id", "arg_lp", "lse"):
        assert np.array_equal(a[k].view(np.uint8), a2[k].view(np.uint8)), k
        assert np.array_equal(a[k][:33].view(np.uint8), b[k][:33].view(np.uint8)), k


@pytest.mark.parametrize("be_name", BACKENDS)
def test_larger_k_and_more_column_steps(be_name):
    be = get_backend(be_name)
    x, w, tg = _inputs(70, 1000, 192)
    bound = _check(_run(be, x, w, tg), x, w, tg, 2e-3)
    assert bound < 6.0e-4                            # the figure 2e-3 was derived from


@pytest.mark.parametrize("be_name", BACKENDS)
def test_just_above_one_slab(be_name):
    """The slab is wider than 1000 columns: N = SLAB + 7 puts seven real columns alone in the second slab.  K = 64: the accumulation bound is
    below the K = 128 case's, so its 1e-3 holds."""
    be = get_backend(be_name)
    x, w, tg = _inputs(70, SLAB + 7, 64)
    tg[:7] = SLAB + np.arange(7)                     # targets in the second slab
    x[40] = 4.0 * w[SLAB + 3]                        # and an argmax there
    bound = _check(_run(be, x, w, tg), x, w, tg, 1e-3)
    assert bound < 2.8e-4
