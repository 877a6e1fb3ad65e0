"""The projection launches of the decode step (engine.hip decode_step: QKV, [Wo | cross-Q], [Wxo | FFN-wi], FFN-wo, lm_head, and the OCR
step's pair with the fp32 epilogue), each in every form the step can launch it in, at operator level: values against a float64 numpy
reference on the bf16-rounded operands, and bits wherever the code promises them (forms that differ only in how the work is cut, and
"a row does not depend on how many rows share its call").

Row counts 1 .. 256 reach the row-tile templates MT = 1 .. 8 of every launcher, both sides of the M > 16 switch and ragged last tiles.
On `hip` the sizes are the benchmark model's (synth.SHAPES["large"]), so that the size-dependent choices are the engine's; on `emu` they are
small, with the long-K (K = 4096) residual form at a narrow N (the emulator runs the whole row list there too: the file costs it seconds).

Tolerances are those of tests/test_kernels.py for the same output kinds: fp32 rtol 1e-4, atol 1e-4 max(1, sqrt(K / 128)); bf16 rtol 1 / 128,
atol 1e-3 (times the output's largest magnitude for the relu output, as test_gemm_pair_product_weights scales it); row sums of the partial
sums of squares rtol 1e-4.

Split mode of the bit comparisons: rows_split_tiles() (k_gemm.hip) cuts gemm_rows / gemm_rows_resid calls over grid.y by WEIGHT SIZE - every
emulator-sized weight would take the one-tile kernels whatever its row count.  The row-count comparisons therefore pin mgk_set_rows_split(0)
(what the benchmark model's 6 - 18 MB weights get by default) and compare modes 1 and -1 against it at every row count: same bits."""
import ctypes as C

import numpy as np
import pytest

from tests import pkutil as pk
from tests.backends import get_backend

BACKENDS = [pytest.param("emu"), pytest.param("hip", marks=pytest.mark.gpu)]
EPI_F32_STORE, EPI_PK_RELU, EPI_HEADS = 0, 2, 4
HF_NONE, HF_STEP_Q, HF_STEP_KV = 0, 4, 5
MG_E_SHAPE = -1

ROWS = [1, 16, 17, 32, 33, 64, 96, 128, 160, 161, 192, 224, 256]
SENT16 = 0xBEEF                 # bf16 -0.4668: "nobody wrote here"
SENT32 = np.float32(-12345.678)
GARBAGE16 = 0x7149              # bf16 ~ 1e30: columns of an activation buffer outside the window a projection reads


def _id(M):
    return "M%d-mt%d" % (M, (M + 31) // 32)


def rows_param(rows=ROWS):
    return pytest.mark.parametrize("M", rows, ids=[_id(m) for m in rows])


def rnd(shape, seed, scale=1.0):
    return (np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32)


def dims(be_name):
    """d, inner, d_ff, V of the benchmark model on hip; emulator sizes otherwise (d_ff: the narrowest N of the whole-tile pair form; kff: the
    long-K residual form)."""
    if be_name == "hip":
        from markushgrapher_amd import synth
        s = synth.SHAPES["large"]
        return dict(d=s.d_model, inner=s.num_heads * 64, dff=s.d_ff, kff=s.d_ff, V=s.vocab_size, narrow=256, T=8)
    return dict(d=64, inner=128, dff=2048, kff=4096, V=1000 + 1, narrow=128, T=8)


def wscale(K):
    return 0.1 if K >= 1024 else 0.3


class ResidDesc(C.Structure):
    _fields_ = [("X", C.c_void_p), ("x_kts", C.c_int), ("x_k0", C.c_int), ("W", C.c_void_p), ("h", C.c_void_p), ("gain", C.c_void_p),
                ("gscale", C.c_float), ("x_pk", C.c_void_p), ("x_ld", C.c_int), ("x_col0", C.c_int), ("x2_pk", C.c_void_p), ("x2_ld", C.c_int),
                ("x2_col0", C.c_int), ("part", C.c_void_p), ("M", C.c_int), ("N", C.c_int), ("K", C.c_int), ("rs_part", C.c_void_p),
                ("rs_nparts", C.c_int), ("rs_inv_d", C.c_float), ("rs_eps", C.c_float), ("wide_tiles", C.c_int), ("alone", C.c_int),
                ("kpart", C.c_void_p), ("ticket", C.c_void_p)]


class ProjDesc(C.Structure):
    _fields_ = [("X", C.c_void_p), ("x_kts", C.c_int), ("x_k0", C.c_int), ("W", C.c_void_p), ("N", C.c_int), ("K", C.c_int),
                ("rs_part", C.c_void_p), ("rs_nparts", C.c_int), ("rs_inv_d", C.c_float), ("rs_eps", C.c_float), ("both_halves", C.c_int),
                ("q", C.c_void_p), ("out_pk", C.c_void_p), ("out_f32", C.c_void_p), ("ldo", C.c_int)]


def ptr(b):
    return b.ptr if b is not None else None


def lib_of(be):
    lib = be.lib
    lib.mgk_gemm_resid_ex.argtypes = [C.c_void_p, C.c_void_p]
    lib.mgk_gemm_pair_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    lib.mgk_gemm_heads_step.argtypes = ([C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p] + [C.c_int] * 3 + [C.c_void_p] * 3 + [C.c_int] * 5 +
                                        [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_int])
    lib.mgk_lm_head_step.argtypes = ([C.c_void_p] * 4 + [C.c_int] * 4 + [C.c_void_p, C.c_int, C.c_float, C.c_float] + [C.c_void_p] * 3 +
                                     [C.c_int, C.c_int])
    return lib


@pytest.fixture(autouse=True)
def _default_switches():
    """Whatever a test did with the process-wide A/B switches, the next one starts from the defaults."""
    yield
    from tests import backends as _b
    for be in _b._cache.values():
        be.lib.mgk_set_rows_split(-1)
        be.lib.mgk_set_rows_ft2(-1)
        be.lib.mgk_set_resid_f16(1)
        be.lib.mgk_set_rows_mt(0)


class Scale:
    """Deferred RMSNorm statistic of 256 rows: partial sums of squares whose row scales r(m) = 1 / sqrt(sum(part[m]) inv_d + eps) spread
    over two orders of magnitude (0.1 .. 10), in an order that has nothing to do with the row index."""

    def __init__(self, be, d, seed):
        rng = np.random.RandomState(seed)
        self.nparts = max(8, d // 8)
        self.inv_d, self.eps = np.float32(1.0 / d), np.float32(1e-6)
        target = 10.0 ** rng.uniform(-1.0, 1.0, 256)                                # r(m)
        cut = rng.uniform(0.5, 1.5, (256, self.nparts))
        self.part = (cut / cut.sum(1, keepdims=True) * (d / target ** 2)[:, None]).astype(np.float32)
        self.r = 1.0 / np.sqrt(self.part.astype(np.float64).sum(1) * np.float64(self.inv_d) + np.float64(self.eps))
        assert self.r.max() / self.r.min() > 30
        self.buf = be.buf(self.part)

    def args(self):
        return self.buf.ptr, self.nparts, float(self.inv_d), float(self.eps)


NO_SCALE = (None, 0, 0.0, 0.0)
_data = {}


def cached(be, key, make):
    """Inputs, references and the 256-row results of a case, made once per backend (the buffers stay alive in here)."""
    k = (be.name,) + key
    if k not in _data:
        _data[k] = make()
    return _data[k]


def bits(a):
    a = np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_bits(a, b, what):
    assert a.shape == b.shape, what
    assert np.array_equal(bits(a), bits(b)), "%s: %d of %d elements differ" % (what, int((bits(a) != bits(b)).sum()), a.size)


def f32_tol(K):
    return dict(rtol=1e-4, atol=1e-4 * max(1.0, np.sqrt(K / 128)))


BF16_TOL = dict(rtol=1 / 128, atol=1e-3)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. QKV
# ---------------------------------------------------------------------------------------------------------------------------------------
def qkv_data(be, D):
    d, inner, T = D["d"], D["inner"], D["T"]
    H = inner // 64
    x, w = rnd((256, d), 1001), rnd((3 * inner, d), 1002, wscale(d))
    rng = np.random.RandomState(1003)
    pos_rows = rng.randint(0, T, 256).astype(np.int32)
    pos_rows[0], pos_rows[1:3] = 0, (T - 1, 0)
    pos_rows[16], pos_rows[31], pos_rows[32], pos_rows[255] = T - 1, 0, T - 1, T - 1
    o = dict(H=H, X=be.buf(pk.pack_tiles(x)), W=be.buf(pk.pack_tiles(w)), rs=Scale(be, d, 1004), pos_rows=pos_rows, POS_ROWS=be.buf(pos_rows))
    o["ref"] = (pk.bf16_round(x).astype(np.float64) @ pk.bf16_round(w).astype(np.float64).T).reshape(256, 3, H, 64)
    return o


def qkv_run(be, D, Q, M, pos=0, pos_dev=None, pos_rows=False, rs=True, both_halves=0):
    lib, H, T = lib_of(be), Q["H"], D["T"]
    Mp = (M + 31) // 32 * 32
    q = be.buf(np.full((Mp, H, 64), SENT16, np.uint16))
    kc = be.buf(np.full((Mp, H, T, 64), SENT16, np.uint16))
    vc = be.buf(np.full((Mp, H, T, 64), SENT16, np.uint16))
    PD = be.buf(np.array([pos_dev], np.int32)) if pos_dev is not None else None
    rc = lib.mgk_gemm_heads_step(be.stream, Q["X"].ptr, 0, 0, Q["W"].ptr, M, 3 * D["inner"], D["d"], q.ptr, kc.ptr, vc.ptr, HF_STEP_Q, HF_STEP_KV,
                                 HF_STEP_KV, H, T, *(Q["rs"].args() if rs else NO_SCALE), pos, ptr(PD), Q["POS_ROWS"].ptr if pos_rows else None,
                                 both_halves)
    assert rc == 0
    return [np.array(a.numpy(), copy=True) for a in (q, kc, vc)]


def cache_rows(c, M, where):
    """the rows a step appended: c[m, :, where[m], :] for m < M; everything else must still hold the sentinel"""
    where = np.asarray(where)
    where = where[:M] if where.ndim else np.full(M, int(where))
    untouched = np.ones(c.shape, bool)
    untouched[np.arange(M), :, where, :] = False
    assert np.all(c[untouched] == SENT16), "the cache changed outside (row, head, position of the row)"
    return c[np.arange(M), :, where, :]


@pytest.mark.parametrize("be_name", BACKENDS)
@rows_param()
def test_qkv_step_projection(be_name, M):
    """The QKV launch: q to [rows][H][64], k / v appended to the cache [rows][H][T_cap][64] at the row's position, which heads_store
    (k_gemm_epi.h) takes from pos_rows[m], else *pos_dev, else pos.  The cache is pre-filled with a sentinel: only (row, head, position of the
    row, :) may change.  Row scales given and not.  both_halves 0 / 1 and the split modes 0 / 1 / default: the same bits; rows [0, M) of the
    256-row call (split mode 0, see the module docstring): the same bits."""
    be = get_backend(be_name)
    D = dims(be_name)
    Q = cached(be, ("qkv",), lambda: qkv_data(be, D))
    T, lib = D["T"], lib_of(be)
    pr = Q["pos_rows"]

    def base(m):
        lib.mgk_set_rows_split(0)
        try:
            q, kc, vc = qkv_run(be, D, Q, m, pos=3, pos_dev=5, pos_rows=True)       # pos_rows wins over both
        finally:
            lib.mgk_set_rows_split(-1)
        assert np.all(q[m:] == SENT16)
        return q[:m], cache_rows(kc, m, pr), cache_rows(vc, m, pr)
    full = cached(be, ("qkv", 256), lambda: base(256))
    got = base(M)
    ref = Q["ref"][:M] * Q["rs"].r[:M, None, None, None]
    for i, name in enumerate("qkv"):
        print("qkv %s M=%d max abs err %.3g" % (name, M, np.abs(pk.bf16_to_f32(got[i]) - ref[:, i]).max()))
        np.testing.assert_allclose(pk.bf16_to_f32(got[i]), ref[:, i], err_msg=name, **BF16_TOL)
        same_bits(got[i], full[i][:M], "%s of rows [0, %d) against the 256-row call" % (name, M))
    # the other ways to cut the same work: same bits
    for split, ft2, bh in ((1, -1, 0), (-1, -1, 0), (0, -1, 1), (0, 1, 0), (0, 0, 1)):
        lib.mgk_set_rows_split(split)
        lib.mgk_set_rows_ft2(ft2)
        try:
            q, kc, vc = qkv_run(be, D, Q, M, pos=3, pos_dev=5, pos_rows=True, both_halves=bh)
        finally:
            lib.mgk_set_rows_split(-1)
            lib.mgk_set_rows_ft2(-1)
        for a, b in zip((q[:M], cache_rows(kc, M, pr), cache_rows(vc, M, pr)), got):
            same_bits(a, b, "split %d ft2 %d both_halves %d" % (split, ft2, bh))
    # the device word wins over the value beside it (graph replay); same numbers, written at that position
    q, kc, vc = qkv_run(be, D, Q, M, pos=1, pos_dev=T - 2)
    same_bits(q[:M], got[0], "q, position from the device word")
    same_bits(cache_rows(kc, M, T - 2), got[1], "k, position from the device word")
    same_bits(cache_rows(vc, M, T - 2), got[2], "v, position from the device word")
    # pos alone, rows already normalised (layer 0)
    q, kc, vc = qkv_run(be, D, Q, M, pos=T - 1, rs=False)
    ref = Q["ref"][:M]
    np.testing.assert_allclose(pk.bf16_to_f32(q[:M]), ref[:, 0], **BF16_TOL)
    np.testing.assert_allclose(pk.bf16_to_f32(cache_rows(kc, M, T - 1)), ref[:, 1], **BF16_TOL)
    np.testing.assert_allclose(pk.bf16_to_f32(cache_rows(vc, M, T - 1)), ref[:, 2], **BF16_TOL)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the residual projection, alone and as the first half of a pair
# ---------------------------------------------------------------------------------------------------------------------------------------
class Resid:
    """h += r(m) X W^T for 256 rows, with whatever of the ResidArgs surface a case asks for.  X is the k-tile window [x_k0, x_k0 + K / 16)
    of a buffer whose other columns hold 1e30 (window=True), x2_pk = bf16(h) the column window [x2_col0, x2_col0 + N) of a sentinel-filled
    buffer, x_pk = bf16(h gain gscale)."""

    def __init__(self, be, N, K, seed, window=True, x2=None, gain=False, gscale=1.0, rs=False, wide_tiles=0):
        self.be, self.N, self.K = be, N, K
        x, w = rnd((256, K), seed), rnd((N, K), seed + 1, wscale(K))
        self.h0 = rnd((256, N), seed + 2)
        self.x_kts, self.x_k0 = ((K + 3 * 64) >> 4, 64 >> 4) if window else (0, 0)
        self.X = be.buf(pk.window_bits(x, K + 3 * 64, 64, GARBAGE16) if window else pk.pack_tiles(x))
        self.W = be.buf(pk.pack_tiles(w))
        self.x2 = x2                                             # (ld, col0) or None
        self.gain = (1 + 0.2 * rnd((N,), seed + 3)) if gain else None
        self.G = be.buf(self.gain) if gain else None
        self.gscale = gscale
        self.rs = Scale(be, N, seed + 4) if rs else None
        self.wide_tiles = wide_tiles
        acc = pk.bf16_round(x).astype(np.float64) @ pk.bf16_round(w).astype(np.float64).T
        self.ref_h = self.h0.astype(np.float64) + acc * (self.rs.r[:, None] if rs else 1.0)

    def desc(self, M, kpart=None, ticket=None, wide_tiles=None):
        be, N = self.be, self.N
        Mp = (M + 31) // 32 * 32
        h = np.full((Mp, N), SENT32, np.float32)
        h[:M] = self.h0[:M]
        self.out = dict(h=be.buf(h), part=be.buf(np.full((Mp, N // 8), SENT32, np.float32)))
        if self.gain is not None:
            self.out["x"] = be.buf(np.full((Mp * N,), SENT16, np.uint16))
        if self.x2:
            self.out["x2"] = be.buf(np.full((Mp * self.x2[0],), SENT16, np.uint16))
        o = self.out
        return ResidDesc(X=self.X.ptr, x_kts=self.x_kts, x_k0=self.x_k0, W=self.W.ptr, h=o["h"].ptr, gain=ptr(self.G), gscale=self.gscale,
                         x_pk=ptr(o.get("x")), x_ld=0, x_col0=0, x2_pk=ptr(o.get("x2")), x2_ld=self.x2[0] if self.x2 else 0,
                         x2_col0=self.x2[1] if self.x2 else 0, part=o["part"].ptr, M=M, N=N, K=self.K,
                         rs_part=self.rs.buf.ptr if self.rs else None, rs_nparts=self.rs.nparts if self.rs else 0,
                         rs_inv_d=self.rs.inv_d if self.rs else 0.0, rs_eps=self.rs.eps if self.rs else 0.0,
                         wide_tiles=self.wide_tiles if wide_tiles is None else wide_tiles, alone=0, kpart=ptr(kpart), ticket=ptr(ticket))

    def collect(self, M):
        """the outputs of the last launch as arrays of M rows, after checking that nothing outside rows [0, M) x the written windows changed"""
        N, o = self.N, self.out
        h, part = np.array(o["h"].numpy(), copy=True), np.array(o["part"].numpy(), copy=True)
        assert np.all(h[M:] == SENT32) and np.all(part[M:] == SENT32), "rows past M were written"
        res = dict(h=h[:M], part=part[:M])
        if "x" in o:
            xb = pk.unpack_tile_bits(o["x"].numpy(), N)
            assert np.all(xb[M:] == SENT16)
            res["x"] = xb[:M].copy()
        if "x2" in o:
            ld, c0 = self.x2
            xb = pk.unpack_tile_bits(o["x2"].numpy(), ld)
            assert np.all(xb[M:] == SENT16) and np.all(xb[:, :c0] == SENT16) and np.all(xb[:, c0 + N:] == SENT16), "x2 written outside its window"
            res["x2"] = xb[:M, c0:c0 + N].copy()
        return res

    def check_values(self, res, M):
        ref = self.ref_h[:M]
        print("resid N=%d K=%d M=%d h max abs err %.3g" % (self.N, self.K, M, np.abs(res["h"] - ref).max()))
        np.testing.assert_allclose(res["h"], ref, **f32_tol(self.K))
        np.testing.assert_allclose(res["part"].astype(np.float64).sum(1), (ref ** 2).sum(1), rtol=1e-4)
        if "x" in res:
            np.testing.assert_allclose(pk.bf16_to_f32(res["x"]), ref * self.gain * self.gscale, **BF16_TOL)
        if "x2" in res:
            np.testing.assert_allclose(pk.bf16_to_f32(res["x2"]), ref, **BF16_TOL)


class Proj:
    """The second half of a pair: its own activation window (the full width K of its buffer), W [N][K], optional row scale."""

    def __init__(self, be, N, K, seed, rs=False):
        self.be, self.N, self.K = be, N, K
        x, w = rnd((256, K), seed), rnd((N, K), seed + 1, wscale(K))
        self.X, self.W = be.buf(pk.pack_tiles(x)), be.buf(pk.pack_tiles(w))
        self.rs = Scale(be, 1024, seed + 2) if rs else None
        self.ref = (pk.bf16_round(x).astype(np.float64) @ pk.bf16_round(w).astype(np.float64).T) * (self.rs.r[:, None] if rs else 1.0)

    def desc(self, M, epi, both_halves):
        be, N = self.be, self.N
        Mp = (M + 31) // 32 * 32
        self.epi = epi
        if epi == EPI_HEADS:
            self.out = be.buf(np.full((Mp, N // 64, 64), SENT16, np.uint16))
        elif epi == EPI_PK_RELU:
            self.out = be.buf(np.full((Mp * N,), SENT16, np.uint16))
        else:
            self.out = be.buf(np.full((Mp, N), SENT32, np.float32))
        return ProjDesc(X=self.X.ptr, x_kts=0, x_k0=0, W=self.W.ptr, N=N, K=self.K, rs_part=self.rs.buf.ptr if self.rs else None,
                        rs_nparts=self.rs.nparts if self.rs else 0, rs_inv_d=self.rs.inv_d if self.rs else 0.0,
                        rs_eps=self.rs.eps if self.rs else 0.0, both_halves=both_halves, q=self.out.ptr if epi == EPI_HEADS else None,
                        out_pk=self.out.ptr if epi == EPI_PK_RELU else None, out_f32=self.out.ptr if epi == EPI_F32_STORE else None, ldo=N)

    def collect(self, M):
        a = np.array(self.out.numpy(), copy=True)
        if self.epi == EPI_PK_RELU:
            a = pk.unpack_tile_bits(a, self.N)
        a = a.reshape(a.shape[0], -1)
        assert np.all(a[M:] == (SENT32 if self.epi == EPI_F32_STORE else SENT16)), "rows past M were written"
        return a[:M]

    def check_values(self, got, M):
        ref = self.ref[:M]
        if self.epi == EPI_F32_STORE:
            np.testing.assert_allclose(got, ref, **f32_tol(self.K))
        elif self.epi == EPI_PK_RELU:
            ref = np.maximum(ref, 0)
            np.testing.assert_allclose(pk.bf16_to_f32(got), ref, rtol=1 / 128, atol=1e-3 * max(1.0, np.abs(ref).max()))
        else:
            np.testing.assert_allclose(pk.bf16_to_f32(got), ref, **BF16_TOL)


def pair_run(be, R, P, M, epi, both_halves=1, resid_f16=1, ft2=-1):
    lib = lib_of(be)
    lib.mgk_set_resid_f16(resid_f16)
    lib.mgk_set_rows_ft2(ft2)
    try:
        rd, pd = R.desc(M), P.desc(M, epi, both_halves)
        assert lib.mgk_gemm_pair_ex(be.stream, C.byref(rd), C.byref(pd), epi) == 0
        res = R.collect(M)
        res["second"] = P.collect(M)
    finally:
        lib.mgk_set_resid_f16(1)
        lib.mgk_set_rows_ft2(-1)
    return res


def pair_case(be, key, make, M, epi, bits_against_256=True):
    R, P = cached(be, key, make)
    res = pair_run(be, R, P, M, epi)
    R.check_values(res, M)
    P.check_values(res["second"], M)
    # the other branches of the dispatch (8-feature residual workgroups, one 16-feature half per workgroup): same bits
    # (both_halves 0 beside 16-feature residual workgroups is what a context that has the GPU to itself launches)
    for bh, f16, ft2 in ((0, 0, 0), (0, 1, -1)):
        other = pair_run(be, R, P, M, epi, both_halves=bh, resid_f16=f16, ft2=ft2)
        for k in res:
            same_bits(res[k], other[k], "%s, both_halves %d resid_f16 %d ft2 %d" % (k, bh, f16, ft2))
    if bits_against_256:
        full = cached(be, key + (256,), lambda: pair_run(be, R, P, 256, epi))
        for k in res:
            same_bits(res[k], full[k][:M], "%s of rows [0, %d) against the 256-row call" % (k, M))


@pytest.mark.parametrize("be_name", BACKENDS)
@rows_param()
def test_wo_cross_q_pair(be_name, M):
    """[Wo | cross-Q], per-head epilogue: the residual half reads the context window of a buffer whose other columns hold 1e30, writes h, the
    partial sums and bf16(h) into a column window of a sentinel-filled buffer; the second half reads the full K2 = d + inner window and
    writes q [rows][H][64].  Forms: one tile (M <= 16), pair_split (17 .. 32), 16-feature residual workgroups (2 tiles on), both 16-feature
    halves per workgroup (3 tiles on, both_halves); mgk_set_resid_f16(0) / mgk_set_rows_ft2(0) take the other branch: same bits.  Rows
    [0, M) of the 256-row call: same bits."""
    be = get_backend(be_name)
    D = dims(be_name)
    d, inner = D["d"], D["inner"]
    pair_case(be, ("woq",), lambda: (Resid(be, d, inner, 2000, x2=(d + inner, inner)), Proj(be, inner, d + inner, 2010)), M, EPI_HEADS)


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("width", ["dff", "narrow"])
@rows_param()
def test_wxo_ffn_wi_pair(be_name, width, M):
    """[Wxo | FFN-wi], packed relu epilogue with the deferred row scale on the second half: N = d_ff takes whole 32-feature tiles per
    workgroup (N >= 2048), the narrow N the half-tile form.  Rows [0, M) of the 256-row call: same bits."""
    be = get_backend(be_name)
    D = dims(be_name)
    d, inner, N = D["d"], D["inner"], D[width]
    pair_case(be, ("wi", width), lambda: (Resid(be, d, inner, 2100), Proj(be, N, d + inner, 2110, rs=True)), M, EPI_PK_RELU)


@pytest.mark.parametrize("be_name", BACKENDS)
@rows_param()
def test_pair_with_fp32_epilogue(be_name, M):
    """The OCR step's pair (ocr.hip: down_proj residual | the next layer's QKV from the product weight): second half with the plain fp32
    store, row stride = N as that call passes it, no gain / packed output on the residual half."""
    be = get_backend(be_name)
    D = dims(be_name)
    d, K = D["d"], D["inner"] * 2
    pair_case(be, ("f32",), lambda: (Resid(be, d, K, 2200), Proj(be, 3 * D["narrow"] // 2, d + K, 2210)), M, EPI_F32_STORE, bits_against_256=False)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. FFN-wo
# ---------------------------------------------------------------------------------------------------------------------------------------
def resid_run(be, R, M, wide_tiles=None, resid_f16=1, split=0, rows_mt=0, kpart=None, ticket=None):
    lib = lib_of(be)
    lib.mgk_set_resid_f16(resid_f16)
    lib.mgk_set_rows_split(split)
    lib.mgk_set_rows_mt(rows_mt)
    try:
        rd = R.desc(M, kpart=kpart, ticket=ticket, wide_tiles=wide_tiles)
        assert lib.mgk_gemm_resid_ex(be.stream, C.byref(rd)) == 0
        return R.collect(M)
    finally:
        lib.mgk_set_resid_f16(1)
        lib.mgk_set_rows_split(-1)
        lib.mgk_set_rows_mt(0)


def ffn_wo(be, D):
    return Resid(be, D["d"], D["kff"], 3000, window=False, x2=(D["d"] + 64, 32), gain=True, gscale=0.5, rs=True, wide_tiles=8)


@pytest.mark.parametrize("be_name", BACKENDS)
@rows_param()
def test_ffn_wo_residual_projection(be_name, M):
    """FFN-wo as the step launches it: K = d_ff, wide_tiles = 8 (16 K-partitioning waves at every row count), row scale, gain, gscale != 1,
    x_pk, x2_pk as a column window, partial sums: resid_split (17 .. 32 rows), <1, 16> (up to 16), <MT, 16, F16> for 2 .. 8 row tiles; the
    8-feature form and the split modes 1 / default: same bits; rows [0, M) of the 256-row call: same bits.  wide_tiles = 0 from five row
    tiles on (the 8-wave form other callers get there) sums K in another partition: values only."""
    be = get_backend(be_name)
    R = cached(be, ("wo2",), lambda: ffn_wo(be, dims(be_name)))
    res = resid_run(be, R, M)
    R.check_values(res, M)
    full = cached(be, ("wo2", 256), lambda: resid_run(be, R, 256))
    for k in res:
        same_bits(res[k], full[k][:M], "%s of rows [0, %d) against the 256-row call" % (k, M))
    for f16, split in ((0, 0), (1, 1), (1, -1)):
        other = resid_run(be, R, M, resid_f16=f16, split=split)
        for k in res:
            same_bits(res[k], other[k], "%s, resid_f16 %d split %d" % (k, f16, split))
    if M > 128:
        R.check_values(resid_run(be, R, M, wide_tiles=0), M)


@pytest.mark.parametrize("be_name", BACKENDS)
def test_ffn_wo_k_slab_form_at_256_rows(be_name):
    """The K-slab form (mgk_set_rows_mt 1: merged by the last arrival; 2: by a second launch) at the largest call, through the entry point the
    other forms are reached by: the same bits as the one-workgroup form, twice on the same scratch, the tickets back at zero."""
    be = get_backend(be_name)
    D = dims(be_name)
    N, K, M = (D["d"], D["kff"], 256) if be_name == "hip" else (256, 512, 256)
    R = cached(be, ("kslab",), lambda: Resid(be, N, K, 3100, window=False, x2=(N + 64, 32), gain=True, gscale=0.5, rs=True, wide_tiles=8))
    res = resid_run(be, R, M)
    R.check_values(res, M)
    kpart, ticket = be.zeros((16 * M * N,), np.float32), be.zeros((N // 32,), np.int32)
    for mode in (1, 1, 2):
        other = resid_run(be, R, M, rows_mt=mode, kpart=kpart, ticket=ticket)
        assert not ticket.numpy().any()
        for k in res:
            same_bits(res[k], other[k], "%s, K-slab mode %d" % (k, mode))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 6. lm_head
# ---------------------------------------------------------------------------------------------------------------------------------------
def lm_data(be, D):
    d, V = D["d"], D["V"]
    Vp = (V + 31) // 32 * 32
    x, w = rnd((256, d), 4000), rnd((V, d), 4001, wscale(d))
    wp = np.zeros((Vp, d), np.float32)
    wp[:V] = w
    wp[V:] = 4.0 * x[:Vp - V]             # weight rows past V that WOULD win rows 0 .. of the last tile if the kernel ranked them
    o = dict(X=be.buf(pk.pack_tiles(x)), W=be.buf(pk.pack_tiles(wp)), rs=Scale(be, d, 4002), Vp=Vp)
    o["ref"] = (pk.bf16_round(x).astype(np.float64) @ pk.bf16_round(w).astype(np.float64).T) * o["rs"].r[:, None]
    top = np.argsort(o["ref"][:2], axis=1)
    o["stops"] = ([int(top[0, -1]), -1, -1, -1], [int(top[0, -1]), int(top[1, -1]), 5, V - 1])      # the winners of rows 0 and 1 among them
    return o


def lm_run(be, D, L, M, top=None, write_logits=1, lse=0):
    lib, V, Vp = lib_of(be), D["V"], L["Vp"]
    P = be.buf(np.full((M, Vp), SENT32, np.float32))
    nt = Vp // 32
    ptop = be.buf(np.full((M, nt, 4), SENT32, np.float32)) if top else None
    stopv = be.buf(np.full((M, 4), SENT32, np.float32)) if top else None
    stop = (C.c_int * 4)(*top) if top else None
    rc = lib.mgk_lm_head_step(be.stream, L["X"].ptr, L["W"].ptr, P.ptr, M, V, D["d"], Vp, *L["rs"].args(), ptr(ptop), ptr(stopv), stop, write_logits,
                              lse)
    assert rc == 0
    return [np.array(a.numpy(), copy=True) if a is not None else None for a in (P, ptop, stopv)]


def check_partials(logits, ptop, stopv, stop, V, lse):
    """top-2 (and the sum of exp(x - best)) of every 32-feature tile from the kernel's OWN fp32 logits, stop tokens and the columns past V
    left out: index and both values exact, the sum to rtol 1e-5"""
    M, Vp = logits.shape[0], ptop.shape[1] * 32
    low = np.float32(-3.0e38)
    x = np.full((M, Vp), low, np.float32)
    x[:, :V] = logits[:, :V]
    for k, s in enumerate(stop):
        if s >= 0:
            same_bits(stopv[:, k], logits[:, s], "stop token %d kept apart" % s)
            x[:, s] = low
        else:
            assert np.all(stopv[:, k] == SENT32)
    t = x.reshape(M, -1, 32)
    i1 = t.argmax(2)
    b1 = np.take_along_axis(t, i1[..., None], 2)[..., 0]
    t2 = t.copy()
    np.put_along_axis(t2, i1[..., None], low, 2)
    b2 = t2.max(2)
    idx = ptop[..., 2].view(np.int32)
    assert idx.max() < V and not np.isin(idx, [s for s in stop if s >= 0]).any()
    assert np.array_equal(idx, i1 + 32 * np.arange(t.shape[1])[None, :])
    same_bits(ptop[..., 0], b1, "best of a tile")
    same_bits(ptop[..., 1], b2, "second of a tile")
    if lse:
        se = np.where(t > low, np.exp(t.astype(np.float64) - b1[..., None].astype(np.float64)), 0.0).sum(2)
        np.testing.assert_allclose(ptop[..., 3], se, rtol=1e-5)
    else:
        assert np.all(ptop[..., 3] == 0)


@pytest.mark.parametrize("be_name", BACKENDS)
@rows_param()
def test_lm_head_step(be_name, M):
    """lm_head as the step launches it (KS = 1, the final norm's row scale, V not a multiple of 32): the plain projection against the
    reference; with TopOut (logits written or not, log-sum-exp terms or not, one and four stop tokens) the partials against the kernel's own
    logits - stop tokens absent from every partial and present in stopv, the columns [V, ldl) of the last tile never ranked although their
    weight rows would win.  Rows [0, M) of the 256-row call: same bits."""
    be = get_backend(be_name)
    D = dims(be_name)
    V = D["V"]
    L = cached(be, ("lm",), lambda: lm_data(be, D))
    one, four = L["stops"]

    def run(m):
        logits = lm_run(be, D, L, m)[0]
        a = lm_run(be, D, L, m, top=one, write_logits=1, lse=1)
        b = lm_run(be, D, L, m, top=four, write_logits=0, lse=0)
        return logits, a, b
    full = cached(be, ("lm", 256), lambda: run(256))
    logits, a, b = run(M)
    assert np.all(logits[:, V:] == SENT32), "logits written past column V"
    print("lm_head M=%d max abs err %.3g" % (M, np.abs(logits[:, :V] - L["ref"][:M]).max()))
    np.testing.assert_allclose(logits[:, :V], L["ref"][:M], **f32_tol(D["d"]))
    same_bits(a[0], logits, "logits beside the partials")
    assert np.all(b[0] == SENT32), "write_logits = 0 wrote logits"
    check_partials(logits, a[1], a[2], one, V, 1)
    check_partials(logits, b[1], b[2], four, V, 0)
    same_bits(logits, full[0][:M], "logits of rows [0, %d) against the 256-row call" % M)
    for got, ref in ((a, full[1]), (b, full[2])):
        same_bits(got[1], ref[1][:M], "partials against the 256-row call")
        same_bits(got[2], ref[2][:M], "stop logits against the 256-row call")


# ---------------------------------------------------------------------------------------------------------------------------------------
# the 256-row limit
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("be_name", BACKENDS)
def test_more_than_256_rows_are_refused(be_name):
    """Eight row tiles is what the launchers are instantiated for: every entry point of the family answers MG_E_SHAPE to 257 rows (and
    launches nothing)."""
    be = get_backend(be_name)
    lib = lib_of(be)
    b = be.zeros((4096,), np.float32)
    p = b.ptr
    lib.mgk_gemm_resid.argtypes = [C.c_void_p] * 5 + [C.c_float] + [C.c_void_p] * 2 + [C.c_int] * 3 + [C.c_void_p, C.c_int, C.c_float, C.c_float]
    lib.mgk_gemm_resid_mt.argtypes = lib.mgk_gemm_resid.argtypes + [C.c_int, C.c_void_p, C.c_void_p]
    lib.mgk_gemm_pair.argtypes = [C.c_void_p] * 4 + [C.c_int] * 3 + [C.c_void_p] * 7 + [C.c_int, C.c_int]
    lib.mgk_lm_head_top.argtypes = [C.c_void_p] * 4 + [C.c_int] * 4 + [C.c_void_p] * 2 + [C.c_int] * 2
    lib.mgk_gemm_splitk.argtypes = [C.c_void_p] * 4 + [C.c_int] * 4 + [C.c_size_t, C.c_int]
    M = 257
    rd = ResidDesc(X=p, W=p, h=p, part=p, M=M, N=64, K=64, gscale=1.0)
    pd = ProjDesc(X=p, W=p, N=64, K=64, q=p, out_pk=p, out_f32=p, ldo=64)
    assert lib.mgk_gemm_resid_ex(be.stream, C.byref(rd)) == MG_E_SHAPE
    for epi in (EPI_HEADS, EPI_PK_RELU, EPI_F32_STORE):
        assert lib.mgk_gemm_pair_ex(be.stream, C.byref(rd), C.byref(pd), epi) == MG_E_SHAPE
    assert lib.mgk_gemm_heads_step(be.stream, p, 0, 0, p, M, 192, 64, p, p, p, HF_STEP_Q, HF_STEP_KV, HF_STEP_KV, 1, 4, None, 0, 0.0, 0.0, 0, None,
                                   None, 0) == MG_E_SHAPE
    stop = (C.c_int * 4)(1, -1, -1, -1)
    assert lib.mgk_lm_head_step(be.stream, p, p, p, M, 64, 64, 64, None, 0, 0.0, 0.0, p, p, stop, 1, 0) == MG_E_SHAPE
    assert lib.mgk_gemm_resid(be.stream, p, p, p, None, 1.0, None, p, M, 64, 64, None, 0, 0.0, 0.0) == MG_E_SHAPE
    assert lib.mgk_gemm_resid_mt(be.stream, p, p, p, None, 1.0, None, p, M, 64, 64, None, 0, 0.0, 0.0, 8, None, None) == MG_E_SHAPE
    assert lib.mgk_gemm_pair(be.stream, p, p, p, 64, 64, 64, p, p, p, p, p, p, p, M, 1) == MG_E_SHAPE
    assert lib.mgk_lm_head_top(be.stream, p, p, p, M, 64, 64, 64, p, p, 1, 0) == MG_E_SHAPE
    assert lib.mgk_gemm_splitk(be.stream, p, p, p, M, 64, 64, 64, 0, 1) == MG_E_SHAPE
    # and what else the new entry points state: K % 64, a window outside its buffer, a row scale the kernels cannot split over 8 threads
    rd = ResidDesc(X=p, W=p, h=p, part=p, M=32, N=64, K=96, gscale=1.0)
    assert lib.mgk_gemm_resid_ex(be.stream, C.byref(rd)) == MG_E_SHAPE
    rd = ResidDesc(X=p, W=p, h=p, part=p, M=32, N=64, K=64, gscale=1.0, x_kts=8, x_k0=6)
    assert lib.mgk_gemm_resid_ex(be.stream, C.byref(rd)) == MG_E_SHAPE
    rd = ResidDesc(X=p, W=p, h=p, part=p, M=32, N=64, K=64, gscale=1.0, x2_pk=p, x2_ld=96, x2_col0=48)
    assert lib.mgk_gemm_resid_ex(be.stream, C.byref(rd)) == MG_E_SHAPE
    rd = ResidDesc(X=p, W=p, h=p, part=p, M=32, N=64, K=64, gscale=1.0, rs_part=p, rs_nparts=4, rs_inv_d=1.0, rs_eps=1e-6)
    assert lib.mgk_gemm_resid_ex(be.stream, C.byref(rd)) == MG_E_SHAPE
