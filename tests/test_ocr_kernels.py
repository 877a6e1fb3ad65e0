"""Operator-level tests of the ChemicalOCR stage's kernels (csrc/k_ocr.hip, the SwiGLU epilogue of the row-streaming GEMM, rmsnorm_pack_tiled,
embed_norm_rows), on the emulator and, marked gpu, on the device - through the test entries mgk_ocr_* / mgk_gemm_swiglu /
mgk_rmsnorm_pack_tiled / mgk_embed_norm_rows.  The arrangement is that of tests/test_swin_kernels.py.

References are float64 numpy restatements of the stock operations (transformers modeling_idefics3.py, modeling_llama.py) on the bf16-rounded
operands.  The restatements that are not obvious are pinned to stock in tests that need no backend: the pixel shuffle to
`Idefics3Connector.pixel_shuffle`, the rotation to `apply_rotary_pos_emb` with `LlamaRotaryEmbedding`, the merge to `inputs_merger`.  Where a
layout or pairing could be exchanged without a symmetric fixture noticing, the case first shows ON THE REFERENCES ALONE that the exchange
moves the result.  Outputs a kernel must not touch are pre-filled with a NaN pattern or a sentinel and checked; nothing is left out of a
comparison except what a kernel is documented not to write.

Tolerances are the project's for the same storage points: bf16-stored outputs rtol 1/128 with atol 1e-3, 2e-3 behind an activation
(tests/test_swin_kernels.py, tests/test_kernels.py); layouts and integer kernels exact; the LayerNorm bound is `ln_bound` of tests/refutil.py
and the RMSNorm bound is built the same way (8x the error of a float32 numpy restatement).  Two are this module's:
  * rotary table: per position band [0, 128), [128, 2048), [2048, 8192), twice the deviation of the STOCK float32 formulation
    (inv_freq = 1 / theta^(i/32) in float32, angle = float32 product, float32 cos / sin) from float64 - the device table rounds the same
    float32 angle (`table_bounds`);
  * rotated Q / K stored in bf16: rtol 1/128 plus that table bound times max|q| of the case.
The device run is the one that counts for the SiLU sites: fast_exp is __expf there and expf on the emulator."""
import ctypes as C
import functools
import math
import types

import numpy as np
import pytest

from tests import pkutil as pk
from tests.backends import get_backend
from tests.refutil import ln_bound

BACKENDS = [pytest.param("emu"), pytest.param("hip", marks=pytest.mark.gpu)]
GPU = pytest.mark.gpu
MG_E_SHAPE, MG_E_UNSUPPORTED = -1, -5
NAN_BITS = 0x7FC1                 # bf16 quiet NaN with a payload: an element the kernel fails to write shows as NaN
SENT = 0xBEEF                     # bf16 bit pattern (-0.4668) that no launch may leave outside its window
ONE = 0x3F80
RTOL = 1.0 / 128
MAX_POS = 8192
GRID_PASS = 65535 * 256           # elements a capped grid of the element-wise kernels covers in one pass


@pytest.fixture(autouse=True)
def _default_rows_switches():
    """Tests that flip the row-streaming GEMM's switches leave the library on its defaults afterwards."""
    yield
    from tests import backends as _b
    for be in _b._cache.values():
        be.lib.mgk_set_rows_split(-1)
        be.lib.mgk_set_rows_ft2(-1)


def _lib(be):
    L = be.lib
    V, I, F = C.c_void_p, C.c_int, C.c_float
    L.mgk_ocr_layernorm_pack.argtypes = [V] * 7 + [I, I, I, F]
    L.mgk_ocr_gelu_pack.argtypes = [V] * 3 + [I] * 3
    L.mgk_ocr_silu_mul_pack.argtypes = [V] * 3 + [I] * 2
    L.mgk_ocr_silu_mul_rows.argtypes = [V, V, V, I, F, F, V, I, I]
    L.mgk_ocr_add_pos.argtypes = [V] * 7 + [I] * 4
    L.mgk_ocr_pixel_shuffle_pack.argtypes = [V] * 3 + [I] * 5
    L.mgk_ocr_merge_embed.argtypes = [V] * 5 + [I] * 7 + [V]
    L.mgk_ocr_rope_heads.argtypes = [V, V] + [I] * 5 + [F] + [V] * 5 + [I]
    L.mgk_ocr_rope_table.argtypes = [V, V, I, F]
    L.mgk_ocr_pack_aug.argtypes = [V, V, V, F, V] + [I] * 6
    L.mgk_ocr_tile_f32.argtypes = [V] * 3 + [I] * 3
    L.mgk_ocr_row_maps.argtypes = [V] * 4 + [I] * 3 + [V]
    L.mgk_ocr_len_delta.argtypes = [V] * 3 + [I, I, V]
    L.mgk_gemm_swiglu.argtypes = [V, V, I, I, V, I, I, I, V, I, F, F, V, I, I]
    L.mgk_rmsnorm_pack_tiled.argtypes = [V] * 5 + [I, I, F]
    L.mgk_embed_norm_rows.argtypes = [V] * 7 + [I] * 5 + [V, F]
    L.mgk_attention_step_rope.argtypes = [V, V, I, V, V, I, F, F, F, V, V, V, I, I, I, I, I, V, I, V, V, V, V, I, I]
    L.mgk_set_rows_split.argtypes = [I]
    L.mgk_set_rows_ft2.argtypes = [I]
    return L


def rs(seed):
    return np.random.RandomState(seed)


def both(cases, device_only=()):
    """the cases on both backends, the device-only ones on the device alone (the emulator walks every lane of every wave on one core)"""
    return [pytest.param("emu", *c) for c in cases] + [pytest.param("hip", *c, marks=GPU) for c in list(cases) + list(device_only)]


def pad32(n):
    return (n + 31) // 32 * 32


def nan_pk(be, rows, K, bits=NAN_BITS):
    return be.buf(np.full((pad32(rows) * K,), bits, np.uint16))


def off_ptr(buf, nbytes):
    return C.c_void_p(buf.ptr + nbytes)


def bf16_expect(ref):
    """the float64 reference, with +-inf where its bf16 rounding overflows (3.39e38 * -3 is -inf in any float32 arithmetic)"""
    with np.errstate(over="ignore"):
        lim = pk.bf16_round(np.asarray(ref, np.float64).astype(np.float32)).astype(np.float64)
    return np.where(np.isinf(lim), lim, ref)


def all_finite_bf16():
    b = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    return pk.bf16_to_f32(b[(b & 0x7F80) != 0x7F80])          # 65280 values: both zeros, the subnormals, up to +-3.39e38


# =====================================================================================================================================
# LayerNorm + pack
# =====================================================================================================================================
def ln_params(d, seed):
    r = rs(seed)
    return (1 + 0.3 * r.standard_normal(d)).astype(np.float32), (0.3 * r.standard_normal(d)).astype(np.float32), \
        r.standard_normal(d).astype(np.float32)


def run_ln(be, x, w, b, eps, Kaug, add_bias=None, want_pk=True, want_f32=True):
    """launch mgk_ocr_layernorm_pack on a copy of x followed by one sentinel row; returns h, out_f32 (each with its sentinel row) and the
    packed bits with their padding rows"""
    L = _lib(be)
    M, d = x.shape
    h = be.buf(np.concatenate([x, np.full((1, d), -77.0, np.float32)]))
    xpk = nan_pk(be, M, Kaug) if want_pk else None
    f32 = be.buf(np.full((M + 1, d), np.nan, np.float32)) if want_f32 else None
    ab = be.buf(add_bias) if add_bias is not None else None
    assert L.mgk_ocr_layernorm_pack(be.stream, be.p(h), be.p(be.buf(w)), be.p(be.buf(b)), be.p(ab), be.p(xpk), be.p(f32), M, d, Kaug, eps) == 0
    o = {"h": h.numpy().copy()}
    if want_pk:
        o["pk"] = pk.unpack_tile_bits(xpk.numpy(), Kaug)
    if want_f32:
        o["f32"] = f32.numpy().copy()
    return o


def check_ln(o, x, ref, bound, Kaug, add_bias, label=None):
    M, d = x.shape
    want_h = x + add_bias if add_bias is not None else x               # float32 add, after the row was read
    assert np.array_equal(o["h"][:M].view(np.uint32), want_h.astype(np.float32).view(np.uint32))
    assert (o["h"][M] == -77.0).all()
    if "f32" in o:
        err = np.abs(o["f32"][:M] - ref)
        if label:
            print(f"{label} out_f32: max err {err.max():.3e}, bound {bound.min():.3e} .. {bound.max():.3e}, max err / bound "
                  f"{(err / np.maximum(bound, 1e-300)).max():.3f}")
        assert (err <= bound).all(), (err / np.maximum(bound, 1e-300)).max()
        assert np.isnan(o["f32"][M]).all()
    if "pk" in o:
        bits = o["pk"]
        assert (bits[M:] == NAN_BITS).all()
        got = pk.bf16_to_f32(bits[:M, :d])
        assert (np.abs(got - ref) <= bound + 2.0 ** -8 * np.abs(ref)).all()
        if Kaug > d:
            assert (bits[:M, d] == ONE).all() and (bits[:M, d + 1:] == 0).all()


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("M", [1, 37, 64])
@pytest.mark.parametrize("d", [64, 80, 128, 768, 1152])
def test_layernorm_pack_widths_and_forms(be_name, d, M):
    """The tower's widths (768, 1152), small ones and one that is not a multiple of 64 x row counts around the 32-row tile x Kaug = d,
    d + 16, d + 64 (the constant-one column at d, zeros behind it) x add_bias (h updated in place after it was read; bit-equal float32 sum)
    x out_f32 alone with x_pk null.  Bound: ln_bound (8x the float32 restatement's own error)."""
    be = get_backend(be_name)
    eps = 1e-6
    r = rs(70 + d + M)
    x = ((0.5 + r.uniform(0, 2, (M, 1))) * r.standard_normal((M, d)) + r.standard_normal((M, 1))).astype(np.float32)
    w, b, ab = ln_params(d, d + 3 * M)
    ref, bound = ln_bound(x, w, b, eps)
    check_ln(run_ln(be, x, w, b, eps, d, add_bias=ab), x, ref, bound, d, ab, label=f"d={d} M={M}")
    check_ln(run_ln(be, x, w, b, eps, d + 16, want_f32=False), x, ref, bound, d + 16, None)
    check_ln(run_ln(be, x, w, b, eps, d + 64, add_bias=ab, want_f32=False), x, ref, bound, d + 64, ab)
    check_ln(run_ln(be, x, w, b, eps, d, want_pk=False), x, ref, bound, d, None)
    check_ln(run_ln(be, x, w, b, eps, d + 16, add_bias=ab, want_pk=False), x, ref, bound, d + 16, ab)


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("d", [64, 80, 768, 1152])
def test_layernorm_pack_rows_that_break_a_careless_kernel(be_name, d):
    """Rows of mean 100 and deviation 0.05 (a one-pass E[x^2] - mean^2 variance in float32 fails on them: asserted on the references alone),
    a constant row (variance 0: the output is b itself), a row of magnitude 1e4 and a row of order 1 with ONE element of 3e4, between
    ordinary rows.  The bound is taken per kind of row."""
    be = get_backend(be_name)
    M, eps = 40, 1e-6
    r = rs(300 + d)
    x = r.standard_normal((M, d)).astype(np.float32)
    x[5] = (1e4 * r.standard_normal(d)).astype(np.float32)
    x[7] = 3.0
    x[10:14] = (100 + 0.05 * r.standard_normal((4, d))).astype(np.float32)
    x[21, d // 3] = 3e4
    x[35] = (100 + 0.05 * r.standard_normal(d)).astype(np.float32)
    w, b, ab = ln_params(d, 17 + d)
    kinds = np.zeros(M, int)
    kinds[5], kinds[7], kinds[10:14], kinds[21], kinds[35] = 1, 2, 3, 4, 3
    ref, bound = ln_bound(x, w, b, eps, kinds)
    x32 = x[10:14]
    m1 = x32.mean(-1, keepdims=True, dtype=np.float32)
    v1 = (x32 * x32).mean(-1, keepdims=True, dtype=np.float32) - m1 * m1
    with np.errstate(invalid="ignore", divide="ignore"):
        one_pass = (x32 - m1) / np.sqrt(v1 + np.float32(eps)) * w + b
    assert not (np.abs(one_pass - ref[10:14]) <= 4 * bound[10:14]).all()
    assert np.array_equal(ref[7], b.astype(np.float64)) and bound[7, 0] == 0      # (3.0 sums exactly in any order: the kernel returns b itself)
    o = run_ln(be, x, w, b, eps, d + 16, add_bias=ab)
    assert np.isfinite(o["f32"][:M]).all()
    err = np.abs(o["f32"][:M] - ref)
    print(f"hard rows d={d}: mean-100 rows max err {err[10:14].max():.3e} (bound {bound[10, 0]:.3e}), 1e4 row {err[5].max():.3e} (bound "
          f"{bound[5, 0]:.3e}), one-huge-element row {err[21].max():.3e} (bound {bound[21, 0]:.3e})")
    check_ln(o, x, ref, bound, d + 16, ab, label=f"hard rows d={d}")
    assert np.array_equal(o["f32"][7], b)


# =====================================================================================================================================
# GELU (tanh) and the three SiLU sites over every finite bf16 value
# =====================================================================================================================================
def gelu_tanh64(x):
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore"):
        return 0.5 * x * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x * x * x)))


def silu64(g):
    g = np.asarray(g, np.float64)
    with np.errstate(over="ignore"):
        return g / (1.0 + np.exp(-g))


def swiglu64(g, u):
    with np.errstate(over="ignore"):
        return silu64(g) * np.asarray(u, np.float64)


def check_activation(got, pre, ref, what):
    """against float64 within the bf16 tolerance behind an activation; no NaN anywhere; finite wherever the exact value is; where the
    exponential of the device overflows or underflows (pre-activation beyond -88) the result is a signed zero or tiny"""
    want = bf16_expect(ref)
    got = np.asarray(got, np.float64)
    assert not np.isnan(got).any(), what
    assert np.isfinite(got[np.isfinite(want)]).all(), what
    with np.errstate(invalid="ignore"):
        bad = ~(np.abs(got - want) <= 2e-3 + RTOL * np.abs(want)) & ~((got == want) & np.isinf(want))
    assert not bad.any(), (what, pre[bad][:4], ref[bad][:4], got[bad][:4])
    deep = pre <= -88
    assert deep.sum() > 100 and (np.abs(got[deep]) <= 1e-34).all(), what


UPS = [1.0, -3.0, 0.007]


@pytest.mark.parametrize("be_name", BACKENDS)
def test_gelu_pack_over_every_finite_bf16_pre_activation(be_name):
    """gelu_pack (torch gelu(approximate="tanh"), SiglipMLP) against float64 on all 65280 finite bf16 values as [272][240] with Kaug = 256:
    the one at column 240, zeros behind it, the padding rows 272 .. 287 untouched.  x^3 overflows float32 from |x| = 7e12 on: tanh(+-inf) =
    +-1 must come out, not NaN."""
    be = get_backend(be_name)
    L = _lib(be)
    vals = all_finite_bf16()
    M, N, Kaug = 272, 240, 256
    assert vals.size == M * N
    pre = rs(1).permutation(vals).reshape(M, N)
    y = nan_pk(be, M, Kaug)
    assert L.mgk_ocr_gelu_pack(be.stream, be.p(be.buf(pre)), be.p(y), M, N, Kaug) == 0
    bits = pk.unpack_tile_bits(y.numpy(), Kaug)
    assert (bits[M:] == NAN_BITS).all() and (bits[:M, N] == ONE).all() and (bits[:M, N + 1:] == 0).all()
    got = pk.bf16_to_f32(bits[:M, :N])
    check_activation(got, pre.astype(np.float64), gelu_tanh64(pre), "gelu_pack")
    assert (got[pre == 0] == 0).all()


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("site", ["silu_mul_pack", "silu_mul_rows"])
def test_silu_sites_over_every_finite_bf16_gate(be_name, site):
    """silu(g) * u with g every finite bf16 value and u in {1, -3, 0.007}, gate / up interleaved, against float64.  Beyond |g| = 88 (and 104,
    where the float32 exponential leaves the normal range) __expf overflows or underflows: g / (1 + inf) is a signed zero, g / (1 + 0) is g."""
    be = get_backend(be_name)
    L = _lib(be)
    vals = all_finite_bf16()
    M, I = 272, 240
    g = rs(2).permutation(vals).reshape(M, I)
    for u in UPS:
        inp = np.empty((M, 2 * I), np.float32)
        inp[:, 0::2], inp[:, 1::2] = g, np.float32(u)
        y = nan_pk(be, M, I)
        if site == "silu_mul_pack":
            assert L.mgk_ocr_silu_mul_pack(be.stream, be.p(be.buf(inp)), be.p(y), M, I) == 0
        else:
            assert L.mgk_ocr_silu_mul_rows(be.stream, be.p(be.buf(inp)), None, 0, 0.0, 0.0, be.p(y), M, I) == 0
        bits = pk.unpack_tile_bits(y.numpy(), I)
        assert (bits[M:] == NAN_BITS).all()
        uu = float(np.float32(u))
        check_activation(pk.bf16_to_f32(bits[:M]), g.astype(np.float64), swiglu64(g, uu), (site, u))


@pytest.mark.parametrize("be_name", BACKENDS)
def test_swiglu_epilogue_over_every_finite_bf16_gate(be_name):
    """The same sweep through the GEMM epilogue: X = one-hot rows, so the accumulator of (m, 2j) is exactly the bf16 value W[2j][m] (the gate)
    and that of (m, 2j + 1) is W[2j + 1][m] (the up value)."""
    be = get_backend(be_name)
    L = _lib(be)
    vals = all_finite_bf16()
    M = K = 64
    I = 1024                                             # 1020 gate rows of 64 values, 4 rows of zeros
    gw = np.zeros((I, K), np.float32)
    gw.reshape(-1)[:vals.size] = rs(3).permutation(vals)
    X = be.buf(pk.pack_tiles(np.eye(M, K, dtype=np.float32)))
    for u in UPS:
        w = np.empty((2 * I, K), np.float32)
        w[0::2], w[1::2] = gw, np.float32(u)
        out = nan_pk(be, M, I)
        assert L.mgk_gemm_swiglu(be.stream, be.p(X), 0, 0, be.p(be.buf(pk.pack_tiles(w))), M, 2 * I, K, None, 0, 0.0, 0.0, be.p(out), 0, 0) == 0
        got = pk.unpack_tiles(out.numpy(), M, I)           # [m][j]: gate gw[j][m]
        pre = gw.T.astype(np.float64)
        check_activation(got, pre, swiglu64(pre, float(np.float32(u))), ("swiglu epilogue", u))


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("M,I", [(1, 256), (37, 1536), (64, 16)])
def test_silu_mul_rows_with_the_deferred_row_scale(be_name, M, I):
    """silu(r g) * (r u) with r = rsqrt(sum(part[m]) * inv_d + eps) per row, against float64; a swapped gate / up pair is shown to move the
    reference beyond 4x the tolerance."""
    be = get_backend(be_name)
    L = _lib(be)
    r = rs(M + I)
    inp = (2.0 * r.standard_normal((M, 2 * I))).astype(np.float32)
    nparts, inv_d, eps = 72, 1.0 / 576, 1e-5
    part = (r.uniform(0.5, 1.5, (M, nparts)) * 8 / r.uniform(0.7, 1.4, (M, 1)) ** 2).astype(np.float32)
    rr = 1.0 / np.sqrt(part.astype(np.float64).sum(-1, keepdims=True) * inv_d + eps)
    g, u = inp[:, 0::2].astype(np.float64) * rr, inp[:, 1::2].astype(np.float64) * rr
    ref = swiglu64(g, u)
    assert (np.abs(swiglu64(u, g) - ref) / (2e-3 + RTOL * np.abs(ref))).max() > 4
    y = nan_pk(be, M, I)
    assert L.mgk_ocr_silu_mul_rows(be.stream, be.p(be.buf(inp)), be.p(be.buf(part)), nparts, inv_d, eps, be.p(y), M, I) == 0
    bits = pk.unpack_tile_bits(y.numpy(), I)
    assert (bits[M:] == NAN_BITS).all()
    np.testing.assert_allclose(pk.bf16_to_f32(bits[:M]), ref, rtol=RTOL, atol=2e-3)


# =====================================================================================================================================
# SwiGLU projection of the decode step; pack_aug
# =====================================================================================================================================
def packed_gate_up(be, gate, up):
    """the interleaved packed weight as the stage builds it: two mgk_ocr_pack_aug calls, gate rows at 0, 2, .., up rows at 1, 3, .."""
    L = _lib(be)
    ti, td = gate.shape
    dst = nan_pk(be, 2 * ti, td)
    for row0, src in ((0, gate), (1, up)):
        assert L.mgk_ocr_pack_aug(be.stream, be.p(be.buf(src)), None, 1.0, be.p(dst), row0, ti, td, td, ti, 2) == 0
    w = np.empty((2 * ti, td), np.float32)
    w[0::2], w[1::2] = gate, up
    assert np.array_equal(dst.numpy(), pk.pack_tiles(w))
    return dst


SWIGLU_M = [1, 20, 32, 45, 70, 128, 256]
SWIGLU_CASES = [(M, 128, 256) for M in SWIGLU_M] + [(1, 576, 1536), (45, 576, 1536)]
SWIGLU_DEVICE = [(M, 576, 1536) for M in SWIGLU_M if M not in (1, 45)]


@pytest.mark.parametrize("be_name,M,td,ti", both(SWIGLU_CASES, SWIGLU_DEVICE))
def test_swiglu_projection(be_name, M, td, ti):
    """gemm_rows with EPI_PK_SWIGLU at 1 .. 8 row tiles: the output as the window [td, td + ti) of a td + ti wide packed buffer and as a plain
    buffer, X as a plain buffer and as the column window [64, 64 + td) of a wider one (NaN in front of it), the deferred RMSNorm scale null
    and given (td / 8 partial sums per row).  Columns [0, td) of the window and rows >= M keep their sentinel.  The row-tile split and the
    both-halves switch give the same bits.  The interleaved weight comes from mgk_ocr_pack_aug (row0 = 0 / 1, rstride = 2); a swapped
    gate / up pair is shown to move the reference beyond 4x the tolerance."""
    be = get_backend(be_name)
    L = _lib(be)
    r = rs(11 * M + td)
    N, K = 2 * ti, td
    x = pk.bf16_round(r.standard_normal((M, K)))
    gate = pk.bf16_round(r.standard_normal((ti, K)) * (2.0 / math.sqrt(K)))
    up = pk.bf16_round(r.standard_normal((ti, K)) * (2.0 / math.sqrt(K)))
    nparts, inv_d, eps = td // 8, 1.0 / td, 1e-5
    scale = r.uniform(0.7, 1.4, (M, 1))
    scale[0] = 0.7
    part = (r.uniform(0.5, 1.5, (M, nparts)) * 8 / scale ** 2).astype(np.float32)
    rr = 1.0 / np.sqrt(part.astype(np.float64).sum(-1, keepdims=True) * inv_d + eps)
    ag, au = x.astype(np.float64) @ gate.astype(np.float64).T, x.astype(np.float64) @ up.astype(np.float64).T
    refs = {False: swiglu64(ag, au), True: swiglu64(ag * rr, au * rr)}
    for k in refs:
        sc = rr if k else 1.0
        assert (np.abs(swiglu64(au * sc, ag * sc) - refs[k]) / (2e-3 + RTOL * np.abs(refs[k]))).max() > 4
    assert (np.abs(refs[True] - refs[False]) / (2e-3 + RTOL * np.abs(refs[False]))).max() > 4            # (the scale is visible)
    W = packed_gate_up(be, gate, up)
    Xp = be.buf(pk.pack_tiles(x))
    xw = np.full((M, K + 64), np.nan, np.float32)
    xw[:, 64:] = x
    Xw = be.buf(pk.pack_tiles(xw))
    PART = be.buf(part)

    def run(out_window, x_window, with_rs):
        ld = td + ti if out_window else ti
        out = nan_pk(be, M, ld, SENT)
        rc = L.mgk_gemm_swiglu(be.stream, be.p(Xw if x_window else Xp), (K + 64) // 16 if x_window else 0, 4 if x_window else 0, be.p(W), M, N, K,
                               be.p(PART) if with_rs else None, nparts if with_rs else 0, inv_d, eps, be.p(out), ld if out_window else 0,
                               td if out_window else 0)
        assert rc == 0
        bits = pk.unpack_tile_bits(out.numpy(), ld).copy()
        assert (bits[M:] == SENT).all()
        if out_window:
            assert (bits[:, :td] == SENT).all()
            bits = bits[:, td:]
        return bits[:M]

    first = None
    for out_window, x_window, with_rs in ((True, True, True), (False, False, False), (True, False, False), (False, True, True)):
        bits = run(out_window, x_window, with_rs)
        got = pk.bf16_to_f32(bits)
        assert np.isfinite(got).all()
        print(f"swiglu M={M} td={td} window={out_window} xwin={x_window} rs={with_rs}: max err / tol = "
              f"{(np.abs(got - refs[with_rs]) / (2e-3 + RTOL * np.abs(refs[with_rs]))).max():.3f}")
        np.testing.assert_allclose(got, refs[with_rs], rtol=RTOL, atol=2e-3)
        if first is None:
            first = bits
    for split in (0, 1):
        L.mgk_set_rows_split(split)
        assert np.array_equal(run(True, True, True), first), ("row-tile split", split)
    L.mgk_set_rows_split(-1)
    for ft2 in (0, 1):
        L.mgk_set_rows_ft2(ft2)
        assert np.array_equal(run(True, True, True), first), ("both halves", ft2)
    L.mgk_set_rows_ft2(-1)


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("N,K,Kaug,Nfill,row0,rstride,bias,scale", [
    (37, 64, 80, 64, 0, 1, True, 1.0), (37, 64, 64, 37, 0, 1, False, 0.125), (20, 48, 64, 32, 1, 2, True, 0.125), (20, 48, 48, 20, 0, 2, False, 1.0),
    (5, 100, 112, 7, 32, 3, True, -2.0)])
def test_pack_aug(be_name, N, K, Kaug, Nfill, row0, rstride, bias, scale):
    """rows row0 + r * rstride <- W[r] * scale | bias[r] * scale at column K | 0; rows N .. Nfill zero; every other row of the destination
    untouched.  Exact (one float32 product, one rounding)."""
    be = get_backend(be_name)
    L = _lib(be)
    r = rs(N + K + Kaug)
    W = r.standard_normal((N, K)).astype(np.float32)
    bv = r.standard_normal(N).astype(np.float32) if bias else None
    rows = pad32(row0 + (Nfill - 1) * rstride + 1 + 3)
    dst = nan_pk(be, rows, Kaug)
    assert L.mgk_ocr_pack_aug(be.stream, be.p(be.buf(W)), be.p(be.buf(bv)) if bias else None, scale, be.p(dst), row0, N, K, Kaug, Nfill, rstride) == 0
    want = np.full((rows, Kaug), NAN_BITS, np.uint16)
    for i in range(Nfill):
        row = np.zeros(Kaug, np.float32)
        if i < N:
            row[:K] = W[i] * np.float32(scale)
            if bias:
                row[K] = bv[i] * np.float32(scale)
        want[row0 + i * rstride] = pk.bf16_bits(row)
    assert np.array_equal(pk.unpack_tile_bits(dst.numpy(), Kaug), want)


# =====================================================================================================================================
# add_pos
# =====================================================================================================================================
def run_add_pos(be, N, P, P_cap, d, ids_kind, with_mask, with_vmask, seed):
    L = _lib(be)
    r = rs(seed)
    patch = r.standard_normal((N, P, d)).astype(np.float32)
    n_pos = P_cap + 5
    pos = pk.bf16_round(r.standard_normal((n_pos, d)))
    if ids_kind is None:
        ids = None
        idx = np.broadcast_to(np.arange(P), (N, P))
    elif ids_kind == "perm":
        ids = np.stack([r.permutation(n_pos)[:P] for _ in range(N)]).astype(np.int32)
        idx = ids
    else:
        ids = r.randint(0, 3, (N, P)).astype(np.int32) * (n_pos // 3)
        idx = ids
    pm = (r.uniform(0, 1, (N, P)) < 0.7).astype(np.uint8) * np.uint8(5) if with_mask else None     # (any non-zero byte attends)
    hidden = be.buf(np.full((N, P_cap, d), np.nan, np.float32))
    vm = be.buf(np.full((N, P_cap), 0xEE, np.uint8)) if with_vmask else None
    assert L.mgk_ocr_add_pos(be.stream, be.p(be.buf(patch)), be.p(be.buf(pk.bf16_bits(pos))), be.p(be.buf(ids)) if ids is not None else None,
                             be.p(be.buf(pm)) if pm is not None else None, be.p(vm), be.p(hidden), N, P, P_cap, d) == 0
    want = np.zeros((N, P_cap, d), np.float32)
    want[:, :P] = patch + pos[idx]                           # one float32 sum
    assert np.array_equal(hidden.numpy().view(np.uint32), want.view(np.uint32))
    if with_vmask:
        wm = np.zeros((N, P_cap), np.uint8)
        wm[:, :P] = (pm != 0) if pm is not None else 1
        assert np.array_equal(vm.numpy(), wm)


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("N,P,P_cap,d,ids_kind,with_mask,with_vmask", [
    (2, 16, 16, 64, None, False, True), (3, 12, 16, 64, "perm", True, True), (2, 12, 32, 80, "rep", False, True),
    (1, 16, 16, 64, "perm", True, False), (3, 9, 16, 48, None, True, True), (2, 16, 16, 768, "rep", True, True)])
def test_add_pos(be_name, N, P, P_cap, d, ids_kind, with_mask, with_vmask):
    """hidden = patch + pos[pos_ids] bit-equal to the float32 sum: P = P_cap and P < P_cap (rows beyond P zero, mask 0), pos_ids null, a
    permutation, repeated ids; patch_mask null / given; vmask null."""
    run_add_pos(get_backend(be_name), N, P, P_cap, d, ids_kind, with_mask, with_vmask, 3 * N + P + d)


# =====================================================================================================================================
# pixel shuffle
# =====================================================================================================================================
def pixel_shuffle_ref(vis, g, sf, mut=None):
    """vis [N][>= g*g][e] -> [N][(g/sf)^2][sf*sf*e]: token (y2, x2), feature (dy*sf + dx)*e + c <- patch (y2*sf + dy)*g + x2*sf + dx.
    `mut` states a wrong kernel: dy / dx exchanged, y2 / x2 exchanged, features ordered channel-major."""
    N, _, e = vis.shape
    g2 = g // sf
    v = vis[:, :g * g].reshape(N, g2, sf, g2, sf, e)          # [n][y2][dy][x2][dx][c]
    order = {None: (0, 1, 3, 2, 4, 5), "dydx": (0, 1, 3, 4, 2, 5), "y2x2": (0, 3, 1, 2, 4, 5), "chan": (0, 1, 3, 5, 2, 4)}[mut]
    return np.ascontiguousarray(v.transpose(order)).reshape(N, g2 * g2, sf * sf * e)


@pytest.mark.parametrize("g,sf", [(4, 2), (8, 4), (32, 4), (6, 3), (8, 2)])
def test_pixel_shuffle_reference_is_stock(g, sf):
    import torch
    from transformers.models.idefics3.modeling_idefics3 import Idefics3Connector
    vis = rs(g + sf).standard_normal((2, g * g, 8))
    stock = Idefics3Connector.pixel_shuffle(None, torch.from_numpy(vis), sf).numpy()
    assert np.array_equal(pixel_shuffle_ref(vis, g, sf), stock)
    for mu in ("dydx", "y2x2", "chan"):
        assert not np.array_equal(pixel_shuffle_ref(vis, g, sf, mu), stock)


def run_pixel_shuffle(be, g, sf, e, N, seed):
    L = _lib(be)
    P_cap = g * g + 7
    vis = rs(seed).standard_normal((N, P_cap, e)).astype(np.float32)
    ref = pixel_shuffle_ref(vis, g, sf)
    T, Fd = (g // sf) ** 2, e * sf * sf
    for mu in ("dydx", "y2x2", "chan"):
        assert (pk.bf16_bits(pixel_shuffle_ref(vis, g, sf, mu)) != pk.bf16_bits(ref)).mean() > 0.25, mu
    out = nan_pk(be, N * T, Fd)
    assert L.mgk_ocr_pixel_shuffle_pack(be.stream, be.p(be.buf(vis)), be.p(out), N, g, P_cap, e, sf) == 0
    bits = pk.unpack_tile_bits(out.numpy(), Fd)
    assert (bits[N * T:] == NAN_BITS).all()
    assert np.array_equal(bits[:N * T], pk.bf16_bits(ref).reshape(N * T, Fd))


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("e", [64, 768])
@pytest.mark.parametrize("g,sf", [(4, 2), (8, 4), (32, 4), (6, 3)])
def test_pixel_shuffle_pack(be_name, g, sf, e, N):
    """bit-equal to the bf16 rounding of the stock shuffle, every patch its own values, P_cap > g * g; before the launch the case shows on
    the references alone that dy / dx exchanged, y2 / x2 exchanged and channel-major features each move the result."""
    run_pixel_shuffle(get_backend(be_name), g, sf, e, N, 100 * g + e + N)


# =====================================================================================================================================
# merge_embed
# =====================================================================================================================================
def merge_ref(ids, tok_emb, feats, T_cap, image_token, per_seq):
    """stock inputs_merger per sequence: the k-th <image> position takes feature row k; an <image> beyond per_seq keeps its own embedding"""
    B, Ln = ids.shape
    d = tok_emb.shape[1]
    h = np.zeros((B, T_cap, d), np.float32)
    for b in range(B):
        k = 0
        for t in range(Ln):
            i = int(ids[b, t])
            im = i == image_token
            if im and feats is not None and k < per_seq:
                h[b, t] = feats[b, k]
            else:
                h[b, t] = tok_emb[i if 0 <= i < tok_emb.shape[0] else 0]
            k += im
    return h


def merge_ids(r, B, Ln, V, image_token, frames, end_at_last=False):
    """`frames` runs of <image> tokens per sequence (lengths given), at random places that differ by sequence, text ids elsewhere"""
    ids = r.randint(0, V - 1, (B, Ln)).astype(np.int64)
    ids[ids == image_token] = image_token + 1
    for b in range(B):
        gaps = Ln - sum(frames)
        cuts = np.sort(r.randint(0, gaps + 1, len(frames)))
        if end_at_last:
            cuts[-1] = gaps
        t = 0
        for f, c0, c1 in zip(frames, np.concatenate([[0], cuts[:-1]]), cuts):
            t += int(c1 - c0)
            ids[b, t:t + f] = image_token
            t += f
    return ids


def test_merge_reference_is_stock():
    import torch
    from transformers.models.idefics3.modeling_idefics3 import Idefics3Model
    r = rs(9)
    B, Ln, V, d, tok, frames = 3, 40, 30, 8, 17, (4, 2, 5)
    ids = merge_ids(r, B, Ln, V, tok, frames)
    emb = r.standard_normal((V, d)).astype(np.float32)
    feats = r.standard_normal((B, sum(frames), d)).astype(np.float32)
    me = types.SimpleNamespace(config=types.SimpleNamespace(image_token_id=tok))
    stock = Idefics3Model.inputs_merger(me, torch.from_numpy(ids), torch.from_numpy(emb[ids]), torch.from_numpy(feats)).numpy()
    assert np.array_equal(merge_ref(ids, emb, feats, Ln, tok, sum(frames)), stock)


def run_merge(be, ids, emb, feats, T_cap, V, tok, per_seq):
    """-> (h, err word); feats sits at the END of its buffer behind a NaN guard, so a read in front of it shows as NaN and on the emulator
    a read behind it leaves the allocation"""
    L = _lib(be)
    B, Ln = ids.shape
    d = emb.shape[1]
    h = be.buf(np.full((B, T_cap, d), np.nan, np.float32))
    err = be.buf(np.zeros(1, np.int32))
    fp = None
    if feats is not None:
        guard = 64
        fb = be.buf(np.concatenate([np.full(guard, np.nan, np.float32), feats.reshape(-1)]))
        fp = off_ptr(fb, guard * 4)
    assert L.mgk_ocr_merge_embed(be.stream, be.p(be.buf(ids)), be.p(be.buf(pk.bf16_bits(emb))), fp, be.p(h), B, Ln, T_cap, d, V, tok, per_seq,
                                 be.p(err)) == 0
    return h.numpy().copy(), int(err.numpy()[0])


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("B,Ln,T_cap,d,frames,with_feats,end_at_last", [
    (3, 70, 96, 64, (9, 4, 9), True, False), (3, 70, 70, 48, (9, 4, 9), False, False), (1, 33, 64, 576, (16,), True, True),
    (3, 2048, 2048, 16, (64, 64, 17), True, True), (2, 2048, 2080, 16, (100,), True, True)])
def test_merge_embed(be_name, B, Ln, T_cap, d, frames, with_feats, end_at_last):
    """several frames per sequence, feats null, T_cap > L (rows zeroed), L = 2048 with <image> tokens ending at position 2047 (the last entry of
    the kernel's rank table), B = 3; bit-equal, error word 0."""
    be = get_backend(be_name)
    r = rs(B + Ln + d)
    V, tok = 300, 211
    ids = merge_ids(r, B, Ln, V, tok, frames, end_at_last)
    if end_at_last:
        assert (ids[:, -1] == tok).all()
    emb = pk.bf16_round(r.standard_normal((V, d)))
    feats = r.standard_normal((B, sum(frames), d)).astype(np.float32) if with_feats else None
    h, err = run_merge(be, ids, emb, feats, T_cap, V, tok, sum(frames))
    want = merge_ref(ids, emb, feats, T_cap, tok, sum(frames))
    assert np.array_equal(h.view(np.uint32), want.view(np.uint32))
    assert err == 0


@pytest.mark.parametrize("be_name", BACKENDS)
def test_merge_embed_error_word(be_name):
    """an id outside [0, V) counts once per id (and reads row 0); a sequence with one <image> too few and one with one too many each count
    once; neither reads outside feats: the missing row is not read, the surplus token keeps its own embedding."""
    be = get_backend(be_name)
    r = rs(77)
    B, Ln, T_cap, d, V, tok, frames = 3, 50, 64, 32, 120, 60, (5, 6)
    per = sum(frames)
    emb = pk.bf16_round(r.standard_normal((V, d)))
    feats = r.standard_normal((B, per, d)).astype(np.float32)
    ids = merge_ids(r, B, Ln, V, tok, frames)
    bad = ids.copy()
    txt = np.argwhere(ids != tok)
    for (b, t), v in zip(txt[[3, 40, 90]], (-1, V, V + 12345678901)):
        bad[b, t] = v
    h, err = run_merge(be, bad, emb, feats, T_cap, V, tok, per)
    assert err == 3
    assert np.array_equal(h.view(np.uint32), merge_ref(bad, emb, feats, T_cap, tok, per).view(np.uint32))
    cnt = ids.copy()
    cnt[0, np.flatnonzero(ids[0] == tok)[2]] = 7                   # sequence 0: one too few
    cnt[2, np.flatnonzero(ids[2] != tok)[-1]] = tok                # sequence 2: one too many, behind the others
    h, err = run_merge(be, cnt, emb, feats, T_cap, V, tok, per)
    assert err == 2
    assert np.array_equal(h.view(np.uint32), merge_ref(cnt, emb, feats, T_cap, tok, per).view(np.uint32))
    h, err = run_merge(be, cnt, emb, None, T_cap, V, tok, per)     # without features the counts are not checked
    assert err == 0


# =====================================================================================================================================
# rotary embedding: the table, the prefill layouts, prefill against decode
# =====================================================================================================================================
BANDS = ((0, 128), (128, 2048), (2048, MAX_POS))
THETAS = [1e4, 1e5]


def inv_freq64(theta):
    return float(theta) ** (-np.arange(32, dtype=np.float64) / 32.0)


def table64(positions, theta):
    ang = np.arange(positions, dtype=np.float64)[:, None] * inv_freq64(theta)[None]
    return np.concatenate([np.cos(ang), np.sin(ang)], 1)


@functools.lru_cache(maxsize=None)
def table_bounds(theta):
    """per position: 2x the deviation of the stock float32 formulation from float64 over the position's band (module docstring)"""
    import torch
    inv = 1.0 / (float(theta) ** (torch.arange(0, 64, 2, dtype=torch.int64).float() / 64))          # LlamaRotaryEmbedding "default"
    ang = torch.arange(MAX_POS, dtype=torch.float32)[:, None] * inv[None]
    stock = torch.cat([ang.cos(), ang.sin()], 1).numpy().astype(np.float64)
    dev = np.abs(stock - table64(MAX_POS, theta)).max(-1)
    out = np.empty(MAX_POS)
    for lo, hi in BANDS:
        out[lo:hi] = 2 * dev[lo:hi].max()
    return out


def rotate64(x, pos, theta, mut=None):
    """stock apply_rotary_pos_emb on [..., 64] at positions `pos` (broadcast over the leading axes): x cos + rotate_half(x) sin, dims i and
    i + 32 pair up.  `mut`: "interleaved" pairs (2i, 2i + 1), "sign" of the sine."""
    ang = np.asarray(pos, np.float64)[..., None] * inv_freq64(theta)
    c, s = np.cos(ang), np.sin(ang)
    if mut == "sign":
        s = -s
    out = np.empty(np.broadcast_shapes(x.shape, c.shape[:-1] + (64,)))
    if mut == "interleaved":
        a, b = x[..., 0::2], x[..., 1::2]
        out[..., 0::2], out[..., 1::2] = a * c - b * s, b * c + a * s
    else:
        a, b = x[..., :32], x[..., 32:]
        out[..., :32], out[..., 32:] = a * c - b * s, b * c + a * s
    return out


@pytest.mark.parametrize("theta", THETAS)
def test_rotation_reference_is_stock(theta):
    import torch
    from transformers import LlamaConfig
    from transformers.models.llama.modeling_llama import LlamaRotaryEmbedding, apply_rotary_pos_emb
    cfg = LlamaConfig(hidden_size=128, num_attention_heads=2, num_key_value_heads=1, max_position_embeddings=MAX_POS, rope_theta=theta)
    rot = LlamaRotaryEmbedding(cfg)
    assert np.allclose(rot.inv_freq.numpy(), inv_freq64(theta), rtol=1e-6)
    T = 48
    r = rs(4)
    q, k = r.standard_normal((1, 2, T, 64)).astype(np.float32), r.standard_normal((1, 1, T, 64)).astype(np.float32)
    cos, sin = rot(torch.from_numpy(q), torch.arange(T)[None])
    qs, ks = apply_rotary_pos_emb(torch.from_numpy(q), torch.from_numpy(k), cos, sin)
    pos = np.arange(T)[None, None, :]
    assert np.abs(rotate64(q.astype(np.float64), pos, theta) - qs.numpy()).max() < 1e-4
    assert np.abs(rotate64(k.astype(np.float64), pos, theta) - ks.numpy()).max() < 1e-4
    for mu in ("interleaved", "sign"):
        assert np.abs(rotate64(q.astype(np.float64), pos, theta, mu) - qs.numpy()).max() > 0.5


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("theta", THETAS)
def test_rope_table(be_name, theta):
    """All 8192 positions against float64; allowed per band: twice the stock float32 formulation's own deviation (stock: 4.5e-6 / 7.2e-5 /
    3.0e-4 at theta 1e4, 6.9e-6 / 1.1e-4 / 4.6e-4 at 1e5).  The kernel takes the inverse frequency as exp2f(-(2i/64) log2f(theta)) in float32
    (relative error up to 4.9e-7 against stock's 7e-8), so its angles differ from stock's by an ulp here and there.
    Measured deviation per band [0, 128) / [128, 2048) / [2048, 8192): MI355X 4.454e-6 / 7.220e-5 / 2.965e-4 at theta 1e4 (stock's own
    figures to the digit) and 7.452e-6 / 1.239e-4 / 4.967e-4 at 1e5 (1.09 of stock's, 0.54 of the allowed); the emulator gives the same
    except 7.467e-6 in the first band at 1e5.  The device's exp2f and sincosf stay inside the margin: no kernel change."""
    be = get_backend(be_name)
    L = _lib(be)
    cs = be.buf(np.full((MAX_POS + 1, 64), np.nan, np.float32))
    assert L.mgk_ocr_rope_table(be.stream, be.p(cs), MAX_POS, theta) == 0
    got = cs.numpy()
    assert np.isnan(got[MAX_POS]).all()
    err = np.abs(got[:MAX_POS].astype(np.float64) - table64(MAX_POS, theta)).max(-1)
    bound = table_bounds(theta)
    for lo, hi in BANDS:
        print(f"rope table {be_name} theta={theta:g} positions [{lo}, {hi}): deviation {err[lo:hi].max():.3e}, allowed {bound[lo]:.3e}")
    assert (err <= bound).all(), [(lo, float(err[lo:hi].max()), float(bound[lo])) for lo, hi in BANDS]


def rope_heads_ref(qkv, B, T, T_cap, H, KV, theta, mut=None):
    """qkv float64 [B*T_cap][(H + 2 KV)*64] -> Q (x 1/8), K, V as [B][H][T_cap][64] with key/value head hh // (H / KV) for query head hh
    (repeat_kv), rows t >= T zero.  `mut`: rotate64's, or "head": key/value head hh % KV."""
    x = qkv.reshape(B, T_cap, H + 2 * KV, 64)
    pos = np.arange(T_cap)[None, :, None]
    rmut = mut if mut in ("interleaved", "sign") else None
    kvh = np.arange(H) % KV if mut == "head" else np.arange(H) // (H // KV)
    q = rotate64(x[:, :, :H], pos, theta, rmut) * 0.125
    k = rotate64(x[:, :, H:H + KV], pos, theta, rmut)[:, :, kvh]
    v = x[:, :, H + KV:][:, :, kvh].copy()
    for a in (q, k, v):
        a[:, T:] = 0
    return q.transpose(0, 2, 1, 3), k.transpose(0, 2, 1, 3), v.transpose(0, 2, 1, 3)


def run_rope_heads(be, B, T, T_cap, H, KV, cap, theta, seed, mutants=True):
    L = _lib(be)
    rep, ld = H // KV, (H + 2 * KV) * 64
    qkv = (1.5 * rs(seed).standard_normal((B * T_cap, ld))).astype(np.float32)         # (rows t >= T hold values too: zeros must be written)
    q, k, v = rope_heads_ref(qkv.astype(np.float64), B, T, T_cap, H, KV, theta)
    bound = table_bounds(theta)[:T_cap][None, None, :, None]
    qa, ka = bound * np.abs(qkv[:, :H * 64]).max() * 0.125, bound * np.abs(qkv[:, H * 64:(H + KV) * 64]).max()
    if mutants:
        muts = ["interleaved", "sign"] + (["head"] if KV > 1 and rep > 1 else [])
        for mu in muts:
            q2, k2, v2 = rope_heads_ref(qkv.astype(np.float64), B, T, T_cap, H, KV, theta, mu)
            moved = max((np.abs(q2 - q) / (qa + RTOL * np.abs(q))).max(), (np.abs(k2 - k) / (ka + RTOL * np.abs(k))).max()) if mu != "head" else \
                (np.abs(k2 - k) / (ka + RTOL * np.abs(k))).max()
            assert moved > 4 and (mu != "head" or not np.array_equal(v2, v)), (mu, moved)
    n = B * H * T_cap * 64
    Q, K, Vt = (be.buf(np.full(n, NAN_BITS, np.uint16)) for _ in range(3))
    Kc, Vc = (be.buf(np.full((B, KV, cap, 64), SENT, np.uint16)) for _ in range(2))
    assert L.mgk_ocr_rope_heads(be.stream, be.p(be.buf(qkv)), B, T, T_cap, H, KV, theta, be.p(Q), be.p(K), be.p(Vt), be.p(Kc), be.p(Vc), cap) == 0
    gq, gk, gv = pk.unpack_heads_rows(Q.numpy(), B, H, T_cap), pk.unpack_heads_rows(K.numpy(), B, H, T_cap), pk.unpack_heads_t(Vt.numpy(), B, H, T_cap)
    for got in (gq, gk, gv):                                   # rows >= T are +0 in every operand: the attention kernel reads whole tiles
        assert (np.ascontiguousarray(got[:, :, T:]).view(np.uint32) == 0).all()
    for name, got, ref, atol in (("Q", gq, q, qa), ("K", gk, k, ka)):
        ratio = np.abs(got - ref) / (atol + RTOL * np.abs(ref) + 1e-300)
        print(f"rope_heads {name} H={H} KV={KV} T={T}: max err / tol = {ratio.max():.3f}")
        assert np.isfinite(got).all() and (ratio <= 1).all(), (name, ratio.max())
    assert np.array_equal(pk.bf16_bits(gv), pk.bf16_bits(v.astype(np.float32)))         # V is rounded, not rotated
    kc, vc = Kc.numpy().reshape(B, KV, cap, 64), Vc.numpy().reshape(B, KV, cap, 64)
    assert (kc[:, :, T:] == SENT).all() and (vc[:, :, T:] == SENT).all()
    assert np.array_equal(kc[:, :, :T], pk.bf16_bits(gk[:, ::rep, :T])) and np.array_equal(vc[:, :, :T], pk.bf16_bits(gv[:, ::rep, :T]))
    for hh in range(H):                                        # repeated heads hold the same bits
        assert np.array_equal(gk[:, hh], gk[:, hh // rep * rep]) and np.array_equal(gv[:, hh], gv[:, hh // rep * rep])


ROPE_HEADS = [(2, 1), (4, 4), (9, 3)]


@pytest.mark.parametrize("be_name,H,KV,B,T,T_cap,cap,theta", both(
    [(H, KV, 2, 70, 96, 128, th) for H, KV in ROPE_HEADS for th in THETAS] + [(9, 3, 1, 96, 96, 100, 1e5), (2, 1, 3, 3, 32, 32, 1e4)],
    [(H, KV, 2, 2000, 2048, 2112, th) for H, KV in ROPE_HEADS for th in THETAS] + [(9, 3, 1, 2048, 2048, 2048, 1e5)]))
def test_rope_heads(be_name, H, KV, B, T, T_cap, cap, theta):
    """Prefill rotation + head layouts against float64: Q carries the 1/8 scale, K does not, V is not rotated; T < T_cap (rows >= T zero in Q,
    K, V^T); key/value heads repeated H / KV times in the packed operands and stored once in the caches; cache rows >= T keep their
    sentinel; cap > T_cap.  Mutants shown on the references first: interleaved pairs (2i, 2i + 1), the sine's sign, head hh % KV."""
    run_rope_heads(get_backend(be_name), B, T, T_cap, H, KV, cap, theta, 13 * H + KV + T)


def ulp_distance(a, b):
    """bf16 bit patterns -> distance in representable values"""
    def key(x):
        x = x.astype(np.int32)
        return np.where(x & 0x8000, -(x & 0x7FFF), x & 0x7FFF)
    return np.abs(key(a) - key(b))


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("theta", THETAS)
def test_prefill_and_decode_write_the_same_cache_rows(be_name, theta):
    """Position t of a cache may come from the prefill (mgk_ocr_rope_heads: sincosf inline) or from a decode step (mgk_attention_step_rope:
    the device's own table, mgk_ocr_rope_table).  The same fp32 q | k | v rows at positions spread over [0, 2048) ([0, 96) on the emulator)
    through both: each is held to the float64 reference (largest error 0.48 of the tolerance, both), V is bit-equal, and so is K.
    Measured: 0 of 11712 elements of K differ in bits on an MI355X at theta 1e4 and at 1e5 (61 positions x 3 heads x 64), 0 of 4224 on the
    emulator: identity is asserted."""
    be = get_backend(be_name)
    L = _lib(be)
    H, KV = 9, 3
    G = H // KV
    T = 2048 if be_name == "hip" else 96
    cap = (T + 63) // 64 * 64 + 64
    ld = (H + 2 * KV) * 64
    qkv = (1.5 * rs(int(theta) % 1000 + T).standard_normal((T, ld))).astype(np.float32)
    pos = np.unique(np.concatenate([[0, 1, 2, 31, 32, 33, 63, 64, T - 2, T - 1], np.linspace(0, T - 1, 48 if be_name == "hip" else 14).astype(int),
                                    [p for p in (127, 128, 129, 1023, 1024, 2047) if p < T]])).astype(np.int32)
    rows = len(pos)
    _, kref, vref = rope_heads_ref(qkv.astype(np.float64), 1, T, T, H, KV, theta)
    kref, vref = kref[0, ::G][:, pos], vref[0, ::G][:, pos]                      # [KV][rows][64]
    katol = table_bounds(theta)[pos][None, :, None] * np.abs(qkv[:, H * 64:(H + KV) * 64]).max()
    # prefill
    n = H * T * 64
    Q, K, Vt = (be.buf(np.zeros(n, np.uint16)) for _ in range(3))
    Kc, Vc = (be.buf(np.full((1, KV, cap, 64), SENT, np.uint16)) for _ in range(2))
    assert L.mgk_ocr_rope_heads(be.stream, be.p(be.buf(qkv)), 1, T, T, H, KV, theta, be.p(Q), be.p(K), be.p(Vt), be.p(Kc), be.p(Vc), cap) == 0
    kp, vp = Kc.numpy().reshape(KV, cap, 64)[:, pos].copy(), Vc.numpy().reshape(KV, cap, 64)[:, pos].copy()
    # decode: one page per position, the row's position from pos_rows
    cs = be.buf(np.zeros((cap, 64), np.float32))
    assert L.mgk_ocr_rope_table(be.stream, be.p(cs), cap, theta) == 0
    Kd, Vd = (be.buf(np.zeros((rows, KV, cap, 64), np.uint16)) for _ in range(2))
    ctx = nan_pk(be, rows, H * 64)
    assert L.mgk_attention_step_rope(be.stream, be.p(be.buf(qkv[pos])), ld, be.p(cs), None, 0, 0.0, 0.0, 0.125, be.p(Kd), be.p(Vd), be.p(ctx), rows,
                                     KV, G, cap, 0, None, 0, be.p(be.buf(pos)), None, None, None, 0, 0) == 0
    ar = np.arange(rows)
    kd = Kd.numpy().reshape(rows, KV, cap, 64)[ar, :, pos].transpose(1, 0, 2)     # [KV][rows][64]
    vd = Vd.numpy().reshape(rows, KV, cap, 64)[ar, :, pos].transpose(1, 0, 2)
    for name, bits in (("prefill", kp), ("decode", kd)):
        got = pk.bf16_to_f32(bits)
        ratio = np.abs(got - kref) / (katol + RTOL * np.abs(kref))
        print(f"{name} K theta={theta:g}: max err / tol = {ratio.max():.3f}")
        assert (ratio <= 1).all(), (name, ratio.max())
    assert np.array_equal(vp, pk.bf16_bits(vref.astype(np.float32))) and np.array_equal(vd, vp)
    dist = ulp_distance(kp, kd)
    print(f"prefill / decode K {be_name} theta={theta:g}: {int((dist != 0).sum())} of {dist.size} elements differ in bits, largest distance "
          f"{int(dist.max())} ulp")
    assert dist.max() == 0


# =====================================================================================================================================
# tile_f32, row_maps, len_delta
# =====================================================================================================================================
@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("M,d", [(32, 4), (96, 64), (64, 576), (32, 1152)])
def test_tile_f32(be_name, M, d):
    """row-major -> tiled is pkutil.tile_f32 bit for bit, and back again returns the rows"""
    be = get_backend(be_name)
    L = _lib(be)
    x = rs(M + d).standard_normal((M, d)).astype(np.float32)
    X = be.buf(x)
    t = be.buf(np.full(M * d, np.nan, np.float32))
    assert L.mgk_ocr_tile_f32(be.stream, be.p(X), be.p(t), M, d, 1) == 0
    assert np.array_equal(t.numpy().view(np.uint32), pk.tile_f32(x).view(np.uint32))
    back = be.buf(np.full((M, d), np.nan, np.float32))
    assert L.mgk_ocr_tile_f32(be.stream, be.p(t), be.p(back), M, d, 0) == 0
    assert np.array_equal(back.numpy().view(np.uint32), x.view(np.uint32))


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("B,T,T_cap,lens", [(3, 37, 64, None), (3, 37, 64, (1, 37, 20)), (2, 32, 32, None), (1, 1, 32, (1,)), (4, 300, 320, (300, 1, 299, 2))])
def test_row_maps(be_name, B, T, T_cap, lens):
    be = get_backend(be_name)
    L = _lib(be)
    last, allr = (be.buf(np.full((B, T_cap), -7, np.int32)) for _ in range(2))
    km = be.buf(np.full((B, T_cap), 0xEE, np.uint8))
    lb = be.buf(np.asarray(lens, np.int32)) if lens is not None else None
    assert L.mgk_ocr_row_maps(be.stream, be.p(last), be.p(allr), be.p(km), B, T, T_cap, be.p(lb)) == 0
    t = np.arange(T_cap)[None]
    ln = np.asarray(lens)[:, None] if lens is not None else np.full((B, 1), T)
    b = np.arange(B)[:, None]
    assert np.array_equal(last.numpy(), np.where(t == ln - 1, b, -1))
    assert np.array_equal(allr.numpy(), np.where(t < T, b * T + t, -1))
    assert np.array_equal(km.numpy(), (t < ln).astype(np.uint8))


@pytest.mark.parametrize("be_name", BACKENDS)
def test_len_delta(be_name):
    be = get_backend(be_name)
    L = _lib(be)
    Ln = 37
    lens = np.array([0, 1, 5, Ln, Ln + 1, -3, 36] + list(range(1, 301)), np.int32)
    delta = be.buf(np.full(lens.size + 1, -777, np.int32))
    err = be.buf(np.zeros(1, np.int32))
    assert L.mgk_ocr_len_delta(be.stream, be.p(be.buf(lens)), be.p(delta), lens.size, Ln, be.p(err)) == 0
    assert np.array_equal(delta.numpy()[:-1], np.clip(lens, 1, Ln) - Ln) and delta.numpy()[-1] == -777
    assert int(err.numpy()[0]) == int(((lens < 1) | (lens > Ln)).sum()) == 3 + 300 - Ln


# =====================================================================================================================================
# rmsnorm_pack_tiled, embed_norm_rows
# =====================================================================================================================================
def rms_ref(x, gain, eps, dtype=np.float64):
    x = x.astype(dtype)
    return x / np.sqrt((x * x).mean(-1, keepdims=True, dtype=dtype) + dtype(eps)) * gain.astype(dtype)


def rms_bound(x, gain, eps):
    """as ln_bound: 8x the largest error of a float32 numpy restatement against float64 on the test's own inputs"""
    ref = rms_ref(x, gain, eps)
    return ref, 8 * np.abs(rms_ref(x, gain, eps, np.float32).astype(np.float64) - ref).max()


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("M", [32, 96])
@pytest.mark.parametrize("d", [128, 576, 1024])
def test_rmsnorm_pack_tiled(be_name, d, M):
    be = get_backend(be_name)
    L = _lib(be)
    r = rs(d + M)
    x = ((0.2 + r.uniform(0, 3, (M, 1))) * r.standard_normal((M, d))).astype(np.float32)
    gain = (1 + 0.3 * r.standard_normal(d)).astype(np.float32)
    eps = 1e-5
    ref, bound = rms_bound(x, gain, eps)
    H, Gn = be.buf(pk.tile_f32(x)), be.buf(gain)
    for want_pk, want_f32 in ((True, True), (True, False), (False, True)):
        xpk = nan_pk(be, M + 32, d) if want_pk else None
        f32 = be.buf(np.full((M + 1, d), np.nan, np.float32)) if want_f32 else None
        assert L.mgk_rmsnorm_pack_tiled(be.stream, be.p(H), be.p(Gn), be.p(xpk), be.p(f32), M, d, eps) == 0
        if want_f32:
            o = f32.numpy()
            print(f"rmsnorm_pack_tiled d={d} M={M}: max err {np.abs(o[:M] - ref).max():.3e}, bound {bound:.3e}")
            assert (np.abs(o[:M] - ref) <= bound).all() and np.isnan(o[M]).all()
        if want_pk:
            bits = pk.unpack_tile_bits(xpk.numpy(), d)
            assert (bits[M:] == NAN_BITS).all()
            assert (np.abs(pk.bf16_to_f32(bits[:M]) - ref) <= bound + 2.0 ** -8 * np.abs(ref)).all()
    assert np.array_equal(H.numpy().view(np.uint32), pk.tile_f32(x).view(np.uint32))


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("with_x2", [False, True])
@pytest.mark.parametrize("d", [128, 576, 1024])
def test_embed_norm_rows(be_name, d, with_x2):
    """h = the embedding row (exact), x_pk = bf16(RMSNorm(h) * gain) against float64, x2 = the row's own bits in its column window; an id out
    of range sets the error word (once per id) and reads row 0."""
    be = get_backend(be_name)
    L = _lib(be)
    r = rs(d + with_x2)
    rows, V, eps = 37, 50, 1e-5
    emb = pk.bf16_round((0.2 + r.uniform(0, 3, (V, 1))) * r.standard_normal((V, d)))
    gain = (1 + 0.3 * r.standard_normal(d)).astype(np.float32)
    ids = r.randint(0, V, rows).astype(np.int64)
    ids[3], ids[5], ids[6] = V + 7, -1, ids[2]
    eff = np.where((ids < 0) | (ids >= V), 0, ids)
    ref, bound = rms_bound(emb[eff], gain, eps)
    h = be.buf(np.full((rows + 1, d), np.nan, np.float32))
    xpk = nan_pk(be, rows, d)
    ld, col0 = d + 64, 40
    x2 = nan_pk(be, rows, ld, SENT) if with_x2 else None
    err = be.buf(np.zeros(1, np.int32))
    assert L.mgk_embed_norm_rows(be.stream, be.p(be.buf(ids)), be.p(be.buf(pk.bf16_bits(emb))), be.p(h), be.p(be.buf(gain)), be.p(xpk), be.p(x2),
                                 ld if with_x2 else 0, col0 if with_x2 else 0, rows, d, V, be.p(err), eps) == 0
    assert int(err.numpy()[0]) == 2
    hh = h.numpy()
    assert np.array_equal(hh[:rows].view(np.uint32), emb[eff].view(np.uint32)) and np.isnan(hh[rows]).all()
    bits = pk.unpack_tile_bits(xpk.numpy(), d)
    assert (bits[rows:] == NAN_BITS).all()
    assert (np.abs(pk.bf16_to_f32(bits[:rows]) - ref) <= bound + 2.0 ** -8 * np.abs(ref)).all()
    if with_x2:
        b2 = pk.unpack_tile_bits(x2.numpy(), ld)
        assert np.array_equal(b2[:rows, col0:col0 + d], pk.bf16_bits(emb[eff]))
        assert (b2[rows:] == SENT).all() and (b2[:, :col0] == SENT).all() and (b2[:, col0 + d:] == SENT).all()


# =====================================================================================================================================
# the second pass of the grid-stride loops (device only)
# =====================================================================================================================================
@GPU
@pytest.mark.parametrize("kernel", ["add_pos", "gelu_pack", "silu_mul_pack", "pixel_shuffle_pack", "rope_heads", "pack_aug", "tile_f32"])
def test_grid_stride_second_pass(kernel):
    """Every element-wise kernel caps its grid at 65535 workgroups of 256 threads and strides; one case per kernel whose element count exceeds
    that (the benchmark's 32 pages: add_pos covers 25.2 M elements), random values that differ in every row, so that a wrong stride or a
    32-bit index shows.  Same references and tolerances as the small cases."""
    be = get_backend("hip")
    L = _lib(be)
    r = rs(len(kernel))
    if kernel == "add_pos":
        assert 32 * 1024 * 768 > GRID_PASS
        run_add_pos(be, 32, 1024, 1024, 768, "perm", True, True, 5)
    elif kernel == "gelu_pack":
        M, N, Kaug = 4100, 4080, 4096
        assert M * Kaug > GRID_PASS
        pre = (3 * r.standard_normal((M, N))).astype(np.float32)
        y = nan_pk(be, M, Kaug)
        assert L.mgk_ocr_gelu_pack(be.stream, be.p(be.buf(pre)), be.p(y), M, N, Kaug) == 0
        bits = pk.unpack_tile_bits(y.numpy(), Kaug)
        assert (bits[M:] == NAN_BITS).all() and (bits[:M, N] == ONE).all() and (bits[:M, N + 1:] == 0).all()
        np.testing.assert_allclose(pk.bf16_to_f32(bits[:M, :N]), gelu_tanh64(pre), rtol=RTOL, atol=2e-3)
    elif kernel == "silu_mul_pack":
        M, I = 4100, 4096
        assert M * I > GRID_PASS
        inp = (3 * r.standard_normal((M, 2 * I))).astype(np.float32)
        y = nan_pk(be, M, I)
        assert L.mgk_ocr_silu_mul_pack(be.stream, be.p(be.buf(inp)), be.p(y), M, I) == 0
        bits = pk.unpack_tile_bits(y.numpy(), I)
        assert (bits[M:] == NAN_BITS).all()
        np.testing.assert_allclose(pk.bf16_to_f32(bits[:M]), swiglu64(inp[:, 0::2], inp[:, 1::2]), rtol=RTOL, atol=2e-3)
    elif kernel == "pixel_shuffle_pack":
        assert 22 * 32 * 32 * 768 > GRID_PASS
        run_pixel_shuffle(be, 32, 4, 768, 22, 6)
    elif kernel == "rope_heads":
        B, T, T_cap, H, KV = 29, 2040, 2048, 9, 3
        assert B * T_cap * H * 32 > GRID_PASS
        run_rope_heads(be, B, T, T_cap, H, KV, T_cap, 1e5, 8, mutants=False)
    elif kernel == "pack_aug":
        N, K, Kaug = 4100, 4096, 4112
        assert N * Kaug > GRID_PASS
        W, bv = r.standard_normal((N, K)).astype(np.float32), r.standard_normal(N).astype(np.float32)
        dst = nan_pk(be, N, Kaug)
        assert L.mgk_ocr_pack_aug(be.stream, be.p(be.buf(W)), be.p(be.buf(bv)), 0.5, be.p(dst), 0, N, K, Kaug, N, 1) == 0
        want = np.full((pad32(N), Kaug), NAN_BITS, np.uint16)
        full = np.zeros((N, Kaug), np.float32)
        full[:, :K], full[:, K] = W * np.float32(0.5), bv * np.float32(0.5)
        want[:N] = pk.bf16_bits(full)
        assert np.array_equal(pk.unpack_tile_bits(dst.numpy(), Kaug), want)
    else:
        M, d = 16416, 4096
        assert M * (d // 4) > GRID_PASS
        x = r.standard_normal((M, d)).astype(np.float32)
        t = be.buf(np.full(M * d, np.nan, np.float32))
        assert L.mgk_ocr_tile_f32(be.stream, be.p(be.buf(x)), be.p(t), M, d, 1) == 0
        assert np.array_equal(t.numpy().view(np.uint32), pk.tile_f32(x).view(np.uint32))
        back = be.buf(np.full((M, d), np.nan, np.float32))
        assert L.mgk_ocr_tile_f32(be.stream, be.p(t), be.p(back), M, d, 0) == 0
        assert np.array_equal(back.numpy().view(np.uint32), x.view(np.uint32))


# =====================================================================================================================================
# argument checks of the entries
# =====================================================================================================================================
def test_entries_reject_what_the_launchers_assume():
    be = get_backend("emu")
    L = _lib(be)
    p = be.p(be.zeros((4096,), np.float32))
    st = be.stream
    assert L.mgk_ocr_layernorm_pack(st, p, p, p, None, p, None, 1, 64, 72, 1e-6) == MG_E_SHAPE            # Kaug % 16
    assert L.mgk_ocr_layernorm_pack(st, p, p, p, None, p, None, 1, 64, 48, 1e-6) == MG_E_SHAPE            # Kaug < d
    assert L.mgk_ocr_layernorm_pack(st, p, p, p, None, None, p, 1, 80, 64, 1e-6) == MG_E_SHAPE            # (also without a packed output)
    assert L.mgk_ocr_layernorm_pack(st, p, p, p, None, None, None, 1, 64, 64, 1e-6) == MG_E_SHAPE         # nothing to write
    assert L.mgk_ocr_gelu_pack(st, p, p, 1, 64, 72) == MG_E_SHAPE and L.mgk_ocr_gelu_pack(st, p, p, 1, 64, 48) == MG_E_SHAPE
    assert L.mgk_ocr_silu_mul_pack(st, p, p, 1, 24) == MG_E_SHAPE
    assert L.mgk_ocr_silu_mul_rows(st, p, None, 0, 0.0, 0.0, p, 1, 24) == MG_E_SHAPE
    assert L.mgk_ocr_silu_mul_rows(st, p, p, 0, 0.0, 0.0, p, 1, 32) == MG_E_SHAPE                          # a scale without partial sums
    assert L.mgk_ocr_add_pos(st, p, p, None, None, None, p, 1, 17, 16, 8) == MG_E_SHAPE                    # P > P_cap
    assert L.mgk_ocr_pixel_shuffle_pack(st, p, p, 1, 6, 36, 16, 4) == MG_E_SHAPE                           # g % sf
    assert L.mgk_ocr_pixel_shuffle_pack(st, p, p, 1, 4, 15, 16, 2) == MG_E_SHAPE                           # P_cap < g * g
    assert L.mgk_ocr_pixel_shuffle_pack(st, p, p, 1, 4, 16, 2, 2) == MG_E_SHAPE                            # e sf^2 % 16
    assert L.mgk_ocr_merge_embed(st, p, p, p, p, 1, 2049, 2080, 4, 10, 3, 1, p) == MG_E_UNSUPPORTED        # the rank table holds 2048 positions
    assert L.mgk_ocr_merge_embed(st, p, p, p, p, 1, 40, 32, 4, 10, 3, 1, p) == MG_E_SHAPE                  # T_cap < L
    assert L.mgk_ocr_rope_heads(st, p, 1, 8, 32, 9, 2, 1e4, p, p, p, p, p, 32) == MG_E_UNSUPPORTED         # H % KV
    assert L.mgk_ocr_rope_heads(st, p, 1, 8, 40, 2, 1, 1e4, p, p, p, p, p, 64) == MG_E_SHAPE               # T_cap % 32
    assert L.mgk_ocr_rope_heads(st, p, 1, 33, 32, 2, 1, 1e4, p, p, p, p, p, 64) == MG_E_SHAPE              # T > T_cap
    assert L.mgk_ocr_rope_heads(st, p, 1, 32, 32, 2, 1, 1e4, p, p, p, p, p, 16) == MG_E_SHAPE              # cap < T
    assert L.mgk_ocr_rope_table(st, p, 0, 1e4) == MG_E_SHAPE and L.mgk_ocr_rope_table(st, p, 8, 0.0) == MG_E_SHAPE
    assert L.mgk_ocr_pack_aug(st, p, None, 1.0, p, 0, 4, 20, 24, 4, 1) == MG_E_SHAPE                       # Kaug % 16
    assert L.mgk_ocr_pack_aug(st, p, p, 1.0, p, 0, 4, 32, 32, 4, 1) == MG_E_SHAPE                          # no column for the bias
    assert L.mgk_ocr_pack_aug(st, p, None, 1.0, p, 0, 4, 32, 32, 3, 1) == MG_E_SHAPE                       # Nfill < N
    assert L.mgk_ocr_tile_f32(st, p, p, 32, 8, 1) == MG_E_SHAPE                                            # in place
    q = be.p(be.zeros((4096,), np.float32))
    assert L.mgk_ocr_tile_f32(st, p, q, 40, 8, 1) == MG_E_SHAPE and L.mgk_ocr_tile_f32(st, p, q, 32, 6, 1) == MG_E_SHAPE
    assert L.mgk_ocr_row_maps(st, p, p, p, 1, 9, 8, None) == MG_E_SHAPE
    assert L.mgk_ocr_len_delta(st, p, p, 0, 4, p) == MG_E_SHAPE
    sw = lambda *a: L.mgk_gemm_swiglu(st, *a)                                                               # noqa: E731
    assert sw(p, 0, 0, p, 257, 64, 64, None, 0, 0.0, 0.0, p, 0, 0) == MG_E_UNSUPPORTED                     # more than 8 row tiles
    assert sw(p, 0, 0, p, 32, 72, 64, None, 0, 0.0, 0.0, p, 64, 0) == MG_E_SHAPE                           # N % 16
    assert sw(p, 0, 0, p, 32, 48, 64, None, 0, 0.0, 0.0, p, 0, 0) == MG_E_SHAPE                            # a plain output of N / 2 = 24 columns
    assert sw(p, 0, 0, p, 32, 64, 96, None, 0, 0.0, 0.0, p, 0, 0) == MG_E_SHAPE                            # K % 64
    assert sw(p, 0, 1, p, 32, 64, 64, None, 0, 0.0, 0.0, p, 0, 0) == MG_E_SHAPE                            # a k-tile offset without a window
    assert sw(p, 6, 3, p, 32, 64, 64, None, 0, 0.0, 0.0, p, 0, 0) == MG_E_SHAPE                            # the window leaves the buffer
    assert sw(p, 0, 0, p, 32, 64, 64, None, 0, 0.0, 0.0, p, 48, 32) == MG_E_SHAPE                          # the output window leaves its buffer
    assert sw(p, 0, 0, p, 32, 64, 64, None, 0, 0.0, 0.0, p, 64, 2) == MG_E_SHAPE                           # out_col0 % 4
    assert sw(p, 0, 0, p, 32, 64, 64, p, 12, 0.0, 0.0, p, 0, 0) == MG_E_SHAPE                              # partial sums not in eights
    assert L.mgk_rmsnorm_pack_tiled(st, p, p, p, None, 40, 64, 1e-5) == MG_E_SHAPE
    assert L.mgk_rmsnorm_pack_tiled(st, p, p, p, None, 32, 72, 1e-5) == MG_E_SHAPE
    assert L.mgk_embed_norm_rows(st, p, p, p, p, p, None, 0, 0, 1, 72, 10, p, 1e-5) == MG_E_SHAPE
    assert L.mgk_embed_norm_rows(st, p, p, p, p, p, p, 96, 36, 1, 64, 10, p, 1e-5) == MG_E_SHAPE           # x2_col0 % 8
    assert L.mgk_embed_norm_rows(st, p, p, p, p, p, p, 96, 40, 1, 64, 10, p, 1e-5) == MG_E_SHAPE           # the window leaves its buffer
