"""The large-M tile GEMM (gemm() in k_gemm.hip / k_gemm_pp.hip, epilogues in k_gemm_epi.h) in every form the encoder, the towers and the
prefill launch it, through the test entry mgk_gemm_ex, against a float64 reference on the bf16-rounded operands.

  per-head forms    EPI_HEADS with the deferred row scale and the row-tile list (encoder QKV from layer 1 on), two launches side by side
                    into one buffer (teacher-forced cross K / V: s_off, S_in != S_cap), one region only (cross Q), HF_NATURAL with row_map
                    and the list (decode cross K / V) - on every tile-kernel variant, K = 64 / 128 / 384, head counts that split a
                    256-column block between the two operand orders;
  schedule forms    the persistent ping-pong kernel's tile schedule (balanced row blocks, column groups, XCD ranges, round-robin, short
                    and empty wave rows, several launches), reached on the real grid with mgk_set_pp_groups; a host restatement of the
                    schedule arithmetic asserts that each case reaches the branch it is named for.

Tolerances are derived per element from the reference (see tol_f32 / tol_bf16): no tuned constants.  Where the code claims "same bits"
(k_gemm.hip gemm(): every tile kernel is the same k-ascending chain of MFMAs; k_gemm_pp.hip; the row-tile list; pp_parts; the group cap)
the outputs are compared bit for bit as well.  Every destination starts as a sentinel bit pattern: what must not be written keeps it."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from tests import pkutil as pk
from tests.backends import get_backend

BACKENDS = [pytest.param("emu"), pytest.param("hip", marks=pytest.mark.gpu)]

EPI_F32_STORE, EPI_F32_RESID, EPI_PK_RELU, EPI_PK, EPI_HEADS, EPI_RESID_NORM = 0, 1, 2, 3, 4, 5
HF_NONE, HF_PK_ROWS, HF_PK_T, HF_NATURAL, HF_STEP_Q = 0, 1, 2, 3, 4
MG_E_SHAPE, MG_E_ARG, MG_E_UNSUPPORTED = -1, -2, -5
SENT = 0xBEEF                                   # bf16 sentinel (a finite value: -0.4668)
SENT_F32 = np.float32(-7.25)
EPS = 1e-6

# Tile-kernel variants (k_gemm.hip): 0 the 128 x 128 kernel, 1 the 256 x 128 kernel, 2 / 4 the 256- / 320-row two-stage kernels, 5 / 6 the
# ping-pong kernel with 256- / 320-row tiles (K % 128 == 0, else the 320-row two-stage kernel), 3 the default (by shape).  Every group is
# compared bit for bit: 5 against 2 and 6 against 4 (k_gemm_pp.hip), and one of the small-tile kernels against each pair (gemm(): "every output
# element is the same k-ascending chain of MFMAs in all tile kernels").
VARIANT_GROUPS = [pytest.param((2, 5, 0), id="v2-5-0"), pytest.param((4, 6, 3, 1), id="v4-6-3-1")]
LIST_VARIANTS = (2, 3, 4, 5, 6)                 # kernels with row-tile list support at M >= 320, N >= 256; 0 / 1 compute every row (mg_kernels.h)


class GemmDesc(C.Structure):
    _fields_ = [("X", C.c_void_p), ("W", C.c_void_p), ("M", C.c_int), ("N", C.c_int), ("K", C.c_int),
                ("out_f32", C.c_void_p), ("ldo", C.c_int), ("bias", C.c_void_p), ("out_pk", C.c_void_p), ("gain", C.c_void_p),
                ("part", C.c_void_p), ("rs_part", C.c_void_p), ("rs_nparts", C.c_int), ("rs_inv_d", C.c_float), ("rs_eps", C.c_float),
                ("head_ptr", C.c_void_p * 3), ("head_fmt", C.c_int * 3), ("H", C.c_int), ("S_in", C.c_int), ("S_cap", C.c_int),
                ("s_off", C.c_int), ("row_map", C.c_void_p), ("row_mask", C.c_void_p), ("list_scratch", C.c_void_p)]


def gemm_ex(be, epi, heads=(), **kw):
    """mgk_gemm_ex with the descriptor's fields from keywords (Buf -> its pointer); heads = up to three (Buf or None, format)."""
    d = GemmDesc()
    for k, v in kw.items():
        setattr(d, k, v.ptr if hasattr(v, "ptr") else v)
    for i, (b, f) in enumerate(heads):
        d.head_ptr[i] = b.ptr if b is not None else None
        d.head_fmt[i] = f
    be.lib.mgk_gemm_ex.argtypes = [C.c_void_p, C.POINTER(GemmDesc), C.c_int]
    be.lib.mgk_gemm_ex.restype = C.c_int
    return be.lib.mgk_gemm_ex(be.stream, C.byref(d), epi)


@pytest.fixture(autouse=True)
def _default_switches():
    """The variant, pp_parts and pp_groups switches are process-wide: back to their defaults after every test, whatever happened in it."""
    yield
    from tests import backends as _b
    for be in _b._cache.values():
        be.lib.mgk_gemm_set_variant(3)
        be.lib.mgk_set_pp_parts(-1)
        be.lib.mgk_set_pp_groups(-1)


# ---------------------------------------------------------------------------------------------------------------------------------------
# reference and tolerances
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def problem(M, N, K, seed=0):
    """Operands (fp32, bf16-exact), the float64 product `ref` and `mag` = (|x| |w|^T) of one GEMM shape; shared and read-only."""
    rs = np.random.RandomState(1000 + seed + M + 7 * N + 13 * K)
    x = pk.bf16_round(rs.standard_normal((M, K)).astype(np.float32))
    w = pk.bf16_round((rs.standard_normal((N, K)) * 0.25).astype(np.float32))
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    ref = x64 @ w64.T
    mag = np.abs(x64) @ np.abs(w64).T
    for a in (x, w, ref, mag):
        a.setflags(write=False)
    return x, w, ref, mag


def tol_f32(K, mag, ref):
    """fp32 outputs: every product of two bf16 values is exact in fp32, the K additions of the MFMA chain each round to fp32 - at most
    K * 2^-24 * sum|x w| - and so does whatever the epilogue adds; twice that, plus one fp32 ulp of the result."""
    return K * 2.0 ** -23 * mag + 2.0 ** -23 * np.abs(ref)


def tol_bf16(K, mag, ref):
    """bf16 outputs (per-head and packed forms): the fp32 bound plus 2^-8 |ref| - the rounding to bf16's 8 significant bits is at most half
    an ulp, 2^-9 to 2^-8 of the value depending on where in its binade it lies.  The fp32 row scale (a sum of <= 20 positive terms, a
    multiply-add and an rsqrt: about 12 * 2^-24 relative at worst) lies within the slack of the fp32 bound, K >= 64."""
    return tol_f32(K, mag, ref) + 2.0 ** -8 * np.abs(ref)


def make_part(M, nparts, K, dead_rows=None, seed=5):
    """Partial sums [M][nparts] as EPI_RESID_NORM leaves them (most of the energy in the late ones: a truncated sum shows), NaN in the rows
    of dead tiles, and the scale r(m) = 1 / sqrt(sum(part[m]) / K + eps) from exactly these values in float64."""
    part = (np.random.RandomState(seed + M + nparts).rand(M, nparts) * 0.5 + 0.25).astype(np.float32)
    part[:, nparts // 2:] *= 9.0
    part[:, nparts - 1] *= 5.0
    r = 1.0 / np.sqrt(part.astype(np.float64).sum(1) / K + EPS)
    if dead_rows is not None:
        part[dead_rows] = np.nan
    return part, r


def close(got, ref, tol, what):
    """|got - ref| <= tol element-wise; prints the worst ratio first (a measurement for whoever reads a failing log)."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    bad = ~(err <= tol)                          # (a NaN fails)
    ratio = float(np.max(err / np.maximum(tol, 1e-300))) if err.size else 0.0
    print("%s: worst |err| / tol = %.3f over %d elements" % (what, ratio, err.size))
    assert not bad.any(), "%s: %d of %d elements out of tolerance, worst |err| / tol = %.3f" % (what, int(bad.sum()), err.size, ratio)


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    ne = a.view(np.uint8) != b.view(np.uint8)
    assert not ne.any(), "%s: %d bytes differ" % (what, int(ne.sum()))


# ---------------------------------------------------------------------------------------------------------------------------------------
# per-head destinations as bit patterns [B][H][S_cap][64] (layouts of mg_kernels.h HeadFmt, restated)
# ---------------------------------------------------------------------------------------------------------------------------------------
def heads_bits(bits, fmt, B, H, S_cap):
    b = np.asarray(bits, np.uint16)
    if fmt == HF_PK_ROWS:                        # [B][H][S_cap/32][4 dim tiles][2 halves][32 tokens][8]
        t = b.reshape(B, H, S_cap // 32, 4, 2, 32, 8).transpose(0, 1, 2, 5, 3, 4, 6)
    elif fmt == HF_PK_T:                         # [B][H][2 dim tiles][S_cap/16][2 halves][32 dims][8 tokens]
        t = b.reshape(B, H, 2, S_cap // 16, 2, 32, 8).transpose(0, 1, 3, 4, 6, 2, 5)
    else:                                        # HF_NATURAL
        t = b.reshape(B, H, S_cap, 64)
    return np.ascontiguousarray(t).reshape(B, H, S_cap, 64)


def token_rows(g):
    """[B][H][S][64] -> [B * S][H][64]: token-major, for S_in = S_cap and s_off = 0."""
    B, H, S, _ = g.shape
    return g.transpose(0, 2, 1, 3).reshape(B * S, H, 64)


def scatter_region(vals, ri, H, B, S_cap, img, dest):
    """Columns [ri * H * 64, (ri + 1) * H * 64) of vals [M][N] -> [B][H][S_cap][64] with token m at (img[m], dest[m]); dest < 0: nowhere."""
    M = vals.shape[0]
    v = vals[:, ri * H * 64:(ri + 1) * H * 64].reshape(M, H, 64)
    out = np.zeros((B, H, S_cap, 64), np.float64)
    keep = dest >= 0
    out[img[keep], :, dest[keep], :] = v[keep]
    return out


def check_heads(got_bits, fmt, ri, H, B, S_cap, img, dest, ref, tol, what):
    """Region ri of a per-head launch: tokens with dest >= 0 hold ref within tol at (img, dest), every other position of the buffer - pad
    rows, dropped rows, dead tiles, another launch's block - holds the sentinel."""
    g = heads_bits(got_bits, fmt, B, H, S_cap)
    written = np.zeros((B, S_cap), bool)
    written[img[dest >= 0], dest[dest >= 0]] = True
    wr = np.broadcast_to(written[:, None, :, None], g.shape)
    assert np.all(g[~wr] == SENT), "%s: %d unwritten elements lost the sentinel" % (what, int((g[~wr] != SENT).sum()))
    R, T = scatter_region(ref, ri, H, B, S_cap, img, dest), scatter_region(tol, ri, H, B, S_cap, img, dest)
    close(pk.bf16_to_f32(g)[wr], R[wr], T[wr], what)


def live_mask(nt, dead):
    live = np.ones(nt, bool)
    live[[t for t in dead if 0 <= t < nt]] = False
    return live


def row_mask_of(live, seed=3):
    """One attended position per live 32-row tile is enough to make it live (row_tile_list, k_attn.hip)."""
    mask = np.zeros(live.size * 32, np.uint8)
    for t in np.nonzero(live)[0]:
        mask[32 * t + (7 * t + seed) % 32] = 1
    return mask


def sent_pk(be, n):
    return be.buf(np.full((n,), SENT, np.uint16))


# ---------------------------------------------------------------------------------------------------------------------------------------
# per-head forms
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("variants", VARIANT_GROUPS)
@pytest.mark.parametrize("K", [64, 128, 384])
@pytest.mark.parametrize("H,B,nparts", [(2, 5, 4), (3, 11, 20)])
def test_heads_qkv_row_scales_and_row_tile_list(be_name, variants, K, H, B, nparts):
    """Encoder QKV from layer 1 on (engine.hip mg_encode): Q, K packed rows, V packed transposed, rows scaled by the deferred RMSNorm scale,
    live row-tile list.  H = 3: a 256-column block holds 192 columns of one region and 64 of the next, so its waves differ in operand order.
    nparts = 20: a second group of 16 partial sums with the clamped re-read in row_scales_tiles.  Dead tiles (NaN in their partial sums)
    inside a block, across the 256-row block boundary and at the end keep the sentinel; live rows are the same bits with and without the
    list, and across the kernels of a variant group."""
    be = get_backend(be_name)
    S, inner = 64, H * 64
    M, N = B * S, 3 * inner
    x, w, ref0, mag0 = problem(M, N, K)
    nt = M // 32
    live = live_mask(nt, [1, 2, 5, 7, 8, 9, 10, nt - 1])      # (block boundaries: tile 8 of the 256-row kernels, 10 of the 320-row ones)
    rowlive = np.repeat(live, 32)
    part, r = make_part(M, nparts, K, dead_rows=~rowlive)
    ref, mag = ref0 * r[:, None], mag0 * r[:, None]
    tol = tol_bf16(K, mag, ref)
    X, W, P = be.buf(pk.pack_tiles(x)), be.buf(pk.pack_tiles(w)), be.buf(part)
    img, s = np.arange(M) // S, np.arange(M) % S
    fmts = (HF_PK_ROWS, HF_PK_ROWS, HF_PK_T)
    first = None
    for v in variants:
        be.lib.mgk_gemm_set_variant(v)
        outs = {}
        for use_list in (True, False):
            q, k, vt = (sent_pk(be, M * inner) for _ in range(3))
            extra = {}
            if use_list:
                scratch = be.zeros((nt + 1,), np.int32)
                extra = dict(row_mask=be.buf(row_mask_of(live)), list_scratch=scratch)
            assert gemm_ex(be, EPI_HEADS, heads=list(zip((q, k, vt), fmts)), X=X, W=W, M=M, N=N, K=K, H=H, S_in=S, S_cap=S,
                           rs_part=P, rs_nparts=nparts, rs_inv_d=1.0 / K, rs_eps=EPS, **extra) == 0
            outs[use_list] = [np.array(b_.numpy(), copy=True) for b_ in (q, k, vt)]
            if use_list:
                sc = scratch.numpy()
                assert sc[0] == live.sum() and np.array_equal(sc[1:1 + sc[0]], np.nonzero(live)[0])
        honoured = v in LIST_VARIANTS
        for ri in range(3):
            got = token_rows(heads_bits(outs[True][ri], fmts[ri], B, H, S))
            if honoured:
                check_heads(outs[True][ri], fmts[ri], ri, H, B, S, img, np.where(rowlive, s, -1), ref, tol, "variant %d region %d" % (v, ri))
            else:                                # every row computed: the live rows are checked, the dead ones are unspecified
                R = ref[:, ri * inner:(ri + 1) * inner].reshape(M, H, 64)[rowlive]
                T = tol[:, ri * inner:(ri + 1) * inner].reshape(M, H, 64)[rowlive]
                close(pk.bf16_to_f32(got[rowlive]), R, T, "variant %d (no list support) region %d" % (v, ri))
            nolist = token_rows(heads_bits(outs[False][ri], fmts[ri], B, H, S))
            same_bits(got[rowlive], nolist[rowlive], "variant %d region %d: list against no list" % (v, ri))
        if first is None:
            first = (v, outs)
        else:
            for ri in range(3):
                a_ = token_rows(heads_bits(first[1][False][ri], fmts[ri], B, H, S))[rowlive]
                b_ = token_rows(heads_bits(outs[False][ri], fmts[ri], B, H, S))[rowlive]
                same_bits(a_, b_, "variant %d against %d, region %d" % (v, first[0], ri))


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("variants", VARIANT_GROUPS)
@pytest.mark.parametrize("K", [64, 128, 384])
@pytest.mark.parametrize("H", [2, 3])
def test_heads_cross_kv_side_by_side(be_name, variants, K, H):
    """Teacher-forced cross K / V (engine.hip decoder_stack): the e1 block (S_in = 64 < S_cap = 192, s_off = 0) and the encoder block
    (S_in = 128, s_off = 64) are two launches into the same packed-rows / packed-transposed buffers.  After each launch the other block is
    untouched: the sentinel after the first, the first launch's bits after the second."""
    be = get_backend(be_name)
    B, S1, S2, S_cap, inner = 5, 64, 128, 192, H * 64
    N = 2 * inner
    M1, M2 = B * S1, B * S2
    x1, w, ref1, mag1 = problem(M1, N, K)
    x2 = problem(M2, N, K, seed=1)[0]
    w64 = w.astype(np.float64)
    ref2, mag2 = x2.astype(np.float64) @ w64.T, np.abs(x2.astype(np.float64)) @ np.abs(w64).T
    X1, X2, W = be.buf(pk.pack_tiles(x1)), be.buf(pk.pack_tiles(x2)), be.buf(pk.pack_tiles(w))
    img1, d1 = np.arange(M1) // S1, np.arange(M1) % S1
    img2, d2 = np.arange(M2) // S2, np.arange(M2) % S2 + S1
    fmts = (HF_PK_ROWS, HF_PK_T)
    first = None
    for v in variants:
        be.lib.mgk_gemm_set_variant(v)
        k, vt = sent_pk(be, B * H * S_cap * 64), sent_pk(be, B * H * S_cap * 64)
        heads = [(k, HF_PK_ROWS), (vt, HF_PK_T), (None, HF_NONE)]
        assert gemm_ex(be, EPI_HEADS, heads=heads, X=X1, W=W, M=M1, N=N, K=K, H=H, S_in=S1, S_cap=S_cap, s_off=0) == 0
        after1 = [np.array(b_.numpy(), copy=True) for b_ in (k, vt)]
        for ri in range(2):                      # (also: the encoder block and nothing else still holds the sentinel)
            check_heads(after1[ri], fmts[ri], ri, H, B, S_cap, img1, d1, ref1, tol_bf16(K, mag1, ref1), "variant %d e1 block, region %d" % (v, ri))
        assert gemm_ex(be, EPI_HEADS, heads=heads, X=X2, W=W, M=M2, N=N, K=K, H=H, S_in=S2, S_cap=S_cap, s_off=S1) == 0
        after2 = [np.array(b_.numpy(), copy=True) for b_ in (k, vt)]
        for ri in range(2):
            a1, a2 = heads_bits(after1[ri], fmts[ri], B, H, S_cap), heads_bits(after2[ri], fmts[ri], B, H, S_cap)
            same_bits(a1[:, :, :S1], a2[:, :, :S1], "variant %d region %d: the e1 block after the encoder launch" % (v, ri))
            assert np.all(a1[:, :, S1:] == SENT)
            close(pk.bf16_to_f32(a2[:, :, S1:]), scatter_region(ref2, ri, H, B, S_cap, img2, d2)[:, :, S1:],
                  scatter_region(tol_bf16(K, mag2, ref2), ri, H, B, S_cap, img2, d2)[:, :, S1:], "variant %d encoder block, region %d" % (v, ri))
        if first is None:
            first = (v, after2)
        else:
            for ri in range(2):
                same_bits(first[1][ri], after2[ri], "variant %d against %d, region %d" % (v, first[0], ri))


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("variants", VARIANT_GROUPS)
@pytest.mark.parametrize("K", [64, 128, 384])
@pytest.mark.parametrize("H", [3, 4])
def test_heads_q_only(be_name, variants, K, H):
    """A projection with one region only (cross-attention Q, engine.hip decoder_stack): N = inner, the other two targets HF_NONE with null
    pointers.  H = 4 reaches the 256-column tile kernels, H = 3 (N = 192) stays below them on every variant.  S_cap = 96 > S_in = 64: the
    pad rows of every (image, head) keep the sentinel."""
    be = get_backend(be_name)
    B, S, S_cap = 11, 64, 96
    M, N = B * S, H * 64
    x, w, ref, mag = problem(M, N, K)
    X, W = be.buf(pk.pack_tiles(x)), be.buf(pk.pack_tiles(w))
    img, s = np.arange(M) // S, np.arange(M) % S
    first = None
    for v in variants:
        be.lib.mgk_gemm_set_variant(v)
        q = sent_pk(be, B * H * S_cap * 64)
        assert gemm_ex(be, EPI_HEADS, heads=[(q, HF_PK_ROWS), (None, HF_NONE), (None, HF_NONE)], X=X, W=W, M=M, N=N, K=K, H=H, S_in=S,
                       S_cap=S_cap) == 0
        got = np.array(q.numpy(), copy=True)
        check_heads(got, HF_PK_ROWS, 0, H, B, S_cap, img, s, ref, tol_bf16(K, mag, ref), "variant %d" % v)
        if first is None:
            first = (v, got)
        else:
            same_bits(first[1], got, "variant %d against %d" % (v, first[0]))


def keep_patterns(B, S, seed):
    """Per image a different keep pattern: everything, nothing, a random half, a prefix that ends inside a tile, whole tiles alternating with
    random ones, ...; destination rows 0 .. n_kept - 1 in token order (embed_assemble's xrow)."""
    rs = np.random.RandomState(seed)
    keep = np.zeros((B, S), bool)
    for b in range(B):
        kind = b % 5
        if kind == 0:
            keep[b] = True
        elif kind == 2:
            keep[b] = rs.rand(S) < 0.5
        elif kind == 3:
            keep[b, :S // 3 + 8] = True
        elif kind == 4:
            for t in range(S // 32):
                if t % 2 == 0:
                    keep[b, 32 * t:32 * t + 32] = rs.rand(32) < 0.3
            keep[b, 5] = True
    dest = np.where(keep, np.cumsum(keep, 1) - 1, -1).astype(np.int32)
    return keep.reshape(-1), dest.reshape(-1)


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("variants", VARIANT_GROUPS)
@pytest.mark.parametrize("K", [64, 128, 384])
@pytest.mark.parametrize("M,S,H", [(640, 128, 2), (1344, 192, 3)])
def test_heads_natural_row_map_and_list(be_name, variants, K, M, S, H):
    """Decode cross K / V (engine.hip cross_kv): HF_NATURAL compacted by row_map, with the live row-tile list at encoder-sized M.  The list
    is consistent with the map (a tile is dead exactly when all its rows are dropped), one image keeps nothing.  Dropped rows - in dead
    tiles and, with the list off, in live ones - and the rows past an image's kept count keep the sentinel; the buffers are the same bits
    with and without the list."""
    be = get_backend(be_name)
    B, inner, S_cap = M // S, H * 64, S + 32
    N = 2 * inner
    x, w, ref, mag = problem(M, N, K)
    tol = tol_bf16(K, mag, ref)
    keep, dest = keep_patterns(B, S, seed=M)
    assert not keep.reshape(B, S)[1].any() and keep.reshape(B, S)[0].all()
    tile_live = keep.reshape(-1, 32).any(1)
    assert (~tile_live).any() and (keep.reshape(-1, 32).any(1) & ~keep.reshape(-1, 32).all(1)).any()      # dead tiles, and live ones with drops
    X, W, RM, MK = be.buf(pk.pack_tiles(x)), be.buf(pk.pack_tiles(w)), be.buf(dest), be.buf(keep.astype(np.uint8))
    img = np.arange(M) // S
    first = None
    for v in variants:
        be.lib.mgk_gemm_set_variant(v)
        outs = {}
        for use_list in (True, False):
            kk, vv = sent_pk(be, B * H * S_cap * 64), sent_pk(be, B * H * S_cap * 64)
            extra = dict(row_mask=MK, list_scratch=be.zeros((M // 32 + 1,), np.int32)) if use_list else {}
            assert gemm_ex(be, EPI_HEADS, heads=[(kk, HF_NATURAL), (vv, HF_NATURAL), (None, HF_NONE)], X=X, W=W, M=M, N=N, K=K, H=H, S_in=S,
                           S_cap=S_cap, row_map=RM, **extra) == 0
            outs[use_list] = [np.array(b_.numpy(), copy=True) for b_ in (kk, vv)]
            for ri in range(2):
                check_heads(outs[use_list][ri], HF_NATURAL, ri, H, B, S_cap, img, dest, ref, tol, "variant %d list %d region %d" % (v, use_list, ri))
        for ri in range(2):
            same_bits(outs[True][ri], outs[False][ri], "variant %d region %d: list against no list" % (v, ri))
        if first is None:
            first = (v, outs[True])
        else:
            for ri in range(2):
                same_bits(first[1][ri], outs[True][ri], "variant %d against %d, region %d" % (v, first[0], ri))


@pytest.mark.parametrize("be_name", BACKENDS)
def test_gemm_ex_refuses_bad_arguments_before_any_device_work(be_name):
    """mgk_gemm_ex validates shapes and nulls first and returns the documented codes (every pointer here is a live buffer or null: a call
    that wrongly went through would still be in bounds)."""
    be = get_backend(be_name)
    M, N, K, H = 64, 128, 64, 2
    X, W = be.zeros((M * K,), np.uint16), be.zeros((N * K,), np.uint16)
    q = be.zeros((M * N,), np.uint16)
    f = be.zeros((M * N,), np.float32)
    part = be.zeros((M, 8), np.float32)
    mask, scratch = be.zeros((M,), np.uint8), be.zeros((M // 32 + 1,), np.int32)
    heads = [(q, HF_PK_ROWS), (None, HF_NONE), (None, HF_NONE)]
    ok = dict(X=X, W=W, M=M, N=N, K=K, H=H, S_in=64, S_cap=64)
    assert gemm_ex(be, EPI_HEADS, heads=heads, **ok) == 0

    def bad(epi=EPI_HEADS, heads=heads, **kw):
        a = dict(ok)
        a.update(kw)
        return gemm_ex(be, epi, heads=heads, **a)
    be.lib.mgk_gemm_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    assert be.lib.mgk_gemm_ex(be.stream, None, EPI_HEADS) == MG_E_ARG
    assert bad(X=None) == MG_E_ARG and bad(W=None) == MG_E_ARG
    assert bad(K=96) == MG_E_SHAPE and bad(K=0) == MG_E_SHAPE and bad(M=0) == MG_E_SHAPE
    assert bad(H=3) == MG_E_SHAPE                                          # N % (H * 64)
    assert bad(H=1, N=256) == MG_E_SHAPE                                   # more than three regions
    assert bad(S_in=64, S_cap=96, s_off=64) == MG_E_SHAPE                  # s_off + S_in <= S_cap
    assert bad(S_in=32, S_cap=96, s_off=16) == MG_E_SHAPE                  # s_off % 32
    assert bad(S_in=32, S_cap=80) == MG_E_SHAPE                            # S_cap % 32 for the packed formats
    assert bad(heads=[(None, HF_PK_ROWS), (None, HF_NONE), (None, HF_NONE)]) == MG_E_ARG      # a region that exists, no target
    assert bad(heads=[(q, HF_STEP_Q), (None, HF_NONE), (None, HF_NONE)]) == MG_E_UNSUPPORTED
    assert bad(heads=[(q, HF_NATURAL), (None, HF_NONE), (None, HF_NONE)], S_in=32, S_cap=64, s_off=32) == MG_E_SHAPE
    assert bad(rs_part=part, rs_nparts=6) == MG_E_SHAPE and bad(rs_part=part, rs_nparts=0) == MG_E_SHAPE      # nparts % 4
    assert bad(row_mask=mask) == MG_E_ARG                                  # a mask and nowhere to build the list
    assert bad(row_mask=mask, list_scratch=scratch, M=48, S_in=48, heads=[(q, HF_NATURAL), (None, HF_NONE), (None, HF_NONE)]) == MG_E_SHAPE
    assert bad(epi=EPI_F32_STORE) == MG_E_ARG and bad(epi=EPI_F32_STORE, out_f32=f, ldo=N - 4) == MG_E_SHAPE
    assert bad(epi=EPI_F32_STORE, out_f32=f, ldo=N, rs_part=part, rs_nparts=8) == MG_E_UNSUPPORTED
    assert bad(epi=EPI_PK) == MG_E_ARG and bad(epi=EPI_PK, out_pk=q, N=120) == MG_E_SHAPE
    assert bad(epi=EPI_RESID_NORM) == MG_E_ARG and bad(epi=EPI_RESID_NORM, out_f32=f, gain=f) == MG_E_ARG
    assert bad(epi=EPI_RESID_NORM, out_f32=f, gain=f, out_pk=q, M=48) == MG_E_SHAPE          # M % 32 with outputs
    assert bad(epi=EPI_RESID_NORM, out_f32=f, part=part, ldo=1) == MG_E_SHAPE               # part_ld < N / 64
    assert bad(epi=EPI_RESID_NORM, out_f32=f, N=112) == MG_E_SHAPE
    assert bad(epi=7) == MG_E_UNSUPPORTED and bad(epi=6) == MG_E_UNSUPPORTED and bad(epi=-1) == MG_E_UNSUPPORTED


# ---------------------------------------------------------------------------------------------------------------------------------------
# The ping-pong kernel's tile schedule, restated on the host (k_gemm_pp.hip: launch_pp and the head of gemm_pp_kernel)
# ---------------------------------------------------------------------------------------------------------------------------------------
GX_N, GP_MAXT, GP_GAIN_MAX = 256, 48, 2048


def pp_schedule(M, N, K, TI, epi, ncu, cap=0, n_list=None, parts_mode=0, colgroup=4, balance=1):
    """None when gemm_pp refuses the shape (the two-stage kernel runs instead); else a dict: G workgroups, and per launch the block grid
    (need -> nbm row blocks x nbn), per workgroup its tiles in order as (bm, bn, in_column_group) and per row block the live row tiles of
    its two wave rows."""
    cdiv = lambda a, b: (a + b - 1) // b
    BM, XT, nbn = 64 * TI, 2 * TI, cdiv(N, GX_N)
    nblk_l = cdiv(M, BM) * nbn
    G = min(nblk_l, ncu)
    if 0 < cap < G:
        G = cap
    if G >= 8:
        G &= ~7
    if K % 128 or (epi == EPI_RESID_NORM and N > GP_GAIN_MAX):
        return None
    parts = 1
    while parts < 8 and cdiv(nblk_l, parts) + cdiv(nblk_l, parts) // 3 + G > GP_MAXT * G:
        parts += 1
    if parts > 1 and (not parts_mode or parts >= 8):
        return None
    if parts < parts_mode <= 8:
        parts = parts_mode
    rt_all = n_list if n_list is not None else cdiv(M, 32)
    launches = []
    for part in range(parts):
        rt0 = part * rt_all // parts if parts > 1 else 0
        nrt = ((part + 1) * rt_all // parts if parts > 1 else rt_all) - rt0
        need = cdiv(nrt, XT)
        step = G // math.gcd(G, nbn)
        bal = cdiv(need, step) * step
        nbm = bal if (balance and bal * 10 <= need * 13 and bal <= nrt) else need
        nblk = nbm * nbn
        T8 = cdiv(nblk, 8)
        wgs = []
        for b in range(G):
            if G % 8 == 0:
                xcd = b & 7
                t_first, t_step, t_end = xcd * T8 + (b >> 3), G >> 3, min((xcd + 1) * T8, nblk)
            else:
                t_first, t_step, t_end = b, G, nblk
            cg_lo = cg_rows = 0
            if colgroup > 0 and G % 8 == 0 and nbn % colgroup == 0 and nbn > colgroup:
                r0, r1 = (b & 7) * T8, min(((b & 7) + 1) * T8, nblk)
                cg_lo = cdiv(r0, nbn) * nbn
                cg_rows = max((r1 // nbn * nbn - cg_lo) // nbn, 0)
            tiles = []
            n_my = min(cdiv(t_end - t_first, t_step), GP_MAXT) if t_first < t_end else 0
            for i in range(n_my):
                tile = t_first + i * t_step
                q = tile - cg_lo
                if cg_rows > 0 and 0 <= q < cg_rows * nbn:
                    per = cg_rows * colgroup
                    g, rem = divmod(q, per)
                    tiles.append((cg_lo // nbn + rem // colgroup, g * colgroup + rem % colgroup, True))
                else:
                    tiles.append((tile // nbn, tile % nbn, False))
            wgs.append(tiles)
        blocks = []
        for bm in range(nbm):
            h = (bm + 1) * nrt // nbm - bm * nrt // nbm
            blocks.append(((h + 1) >> 1, h - ((h + 1) >> 1)))
        launches.append(dict(nrt=nrt, need=need, nbm=nbm, nbn=nbn, wgs=wgs, blocks=blocks))
    return dict(G=G, TI=TI, parts=parts, launches=launches)


def pp_summary(s):
    """The branches a schedule reaches, and a check of the restatement itself: every block of every launch is some workgroup's tile once."""
    out = dict(G=s["G"], parts=s["parts"], tiles=0, cg_tiles=0, linear_tiles=0, per_wg=[], balanced=False, short=False, empty_row=False,
               xcd=s["G"] % 8 == 0)
    for L in s["launches"]:
        seen = sorted((bm, bn) for t in L["wgs"] for bm, bn, _ in t)
        assert seen == [(bm, bn) for bm in range(L["nbm"]) for bn in range(L["nbn"])]
        out["tiles"] += len(seen)
        out["cg_tiles"] += sum(cg for t in L["wgs"] for _, _, cg in t)
        out["per_wg"] += [len(t) for t in L["wgs"]]
        out["balanced"] |= L["nbm"] != L["need"]
        out["short"] |= any(0 < c < s["TI"] for blk in L["blocks"] for c in blk)
        out["empty_row"] |= any(c == 0 for blk in L["blocks"] for c in blk)
        assert all(c <= s["TI"] for blk in L["blocks"] for c in blk)
    out["linear_tiles"] = out["tiles"] - out["cg_tiles"]
    return out


def ncu_of(be):
    return 8 if be.name == "emu" else be.torch.cuda.get_device_properties(0).multi_processor_count


def run_epi(be, epi, X, W, M, N, K, ops, extra):
    """One launch of epilogue `epi` into fresh sentinel-filled outputs; returns them as host arrays (by name)."""
    Mp = (M + 31) // 32 * 32
    if epi in (EPI_PK, EPI_PK_RELU):
        o = sent_pk(be, Mp * N)
        assert gemm_ex(be, epi, X=X, W=W, M=M, N=N, K=K, out_pk=o, **extra) == 0
        return dict(out_pk=np.array(o.numpy(), copy=True))
    if epi == EPI_RESID_NORM:
        h, xo = be.buf(ops["h0_tiled"]), sent_pk(be, Mp * N)
        part = be.buf(np.full((Mp, ops["np4"]), SENT_F32, np.float32))
        assert gemm_ex(be, epi, X=X, W=W, M=M, N=N, K=K, out_f32=h, gain=ops["G"], out_pk=xo, part=part, ldo=ops["np4"], **extra) == 0
        return dict(h=np.array(h.numpy(), copy=True), x_pk=np.array(xo.numpy(), copy=True), part=np.array(part.numpy(), copy=True))
    Hh = ops["H"]
    q, k, vt = (sent_pk(be, Mp * Hh * 64) for _ in range(3))
    heads = list(zip((q, k, vt), (HF_PK_ROWS, HF_PK_ROWS, HF_PK_T)))[:N // (Hh * 64)] + [(None, HF_NONE)] * (3 - N // (Hh * 64))
    assert gemm_ex(be, EPI_HEADS, heads=heads, X=X, W=W, M=M, N=N, K=K, H=Hh, S_in=32, S_cap=32, **extra) == 0
    return {"heads%d" % i: np.array(b_.numpy(), copy=True) for i, b_ in enumerate((q, k, vt)[:N // (Hh * 64)])}


def check_epi(epi, res, M, N, K, ops, rowlive, what, relu=False):
    """The outputs of run_epi against the float64 reference on live rows; dead rows keep what was there before."""
    x, w, ref, mag = problem(M, N, K)
    if epi in (EPI_PK, EPI_PK_RELU):
        bits = pk.unpack_tile_bits(res["out_pk"], N)[:M]
        assert np.all(bits[~rowlive] == SENT), what
        r_ = np.maximum(ref, 0) if epi == EPI_PK_RELU else ref
        close(pk.bf16_to_f32(bits[rowlive]), r_[rowlive], tol_bf16(K, mag, ref)[rowlive], what + " packed")
    elif epi == EPI_RESID_NORM:
        h0, g = ops["h0"].astype(np.float64), ops["g"].astype(np.float64)
        href = h0 + ref
        # the accumulator bound, one more fp32 rounding for the addition of h0 (2^-24 of the result, inside the 2^-23 |ref| term of a result
        # that now includes h0)
        th = K * 2.0 ** -23 * mag + 2.0 ** -23 * np.abs(href)
        h = pk.untile_f32(res["h"], N)[:M]
        same_bits(h[~rowlive], ops["h0"][~rowlive], what + ": dead rows of h")
        close(h[rowlive], href[rowlive], th[rowlive], what + " h")
        xb = pk.unpack_tile_bits(res["x_pk"], N)[:M]
        assert np.all(xb[~rowlive] == SENT), what
        xr = href * g
        close(pk.bf16_to_f32(xb[rowlive]), xr[rowlive], (th * np.abs(g) + 2.0 ** -8 * np.abs(xr))[rowlive], what + " bf16(h gain)")
        # part[m][j] = sum of h^2 over columns [64 j, 64 j + 64): 64 squares and 63 additions in fp32, all terms positive (<= 128 roundings of
        # 2^-24 relative), plus the error of h itself, 2 |h| th to first order
        p = res["part"][:M, :N // 64]
        pr = (href ** 2).reshape(M, N // 64, 64).sum(2)
        tp = (2 * np.abs(href) * th).reshape(M, N // 64, 64).sum(2) + 128 * 2.0 ** -24 * pr
        assert np.all(res["part"][:M][~rowlive] == SENT_F32) and np.all(res["part"][:M, N // 64:] == SENT_F32), what
        close(p[rowlive], pr[rowlive], tp[rowlive], what + " partial sums")
    else:
        Hh = ops["H"]
        B, img, dest = M // 32, np.arange(M) // 32, np.where(rowlive, np.arange(M) % 32, -1)
        for i in range(N // (Hh * 64)):
            check_heads(res["heads%d" % i], HF_PK_T if i == 2 else HF_PK_ROWS, i, Hh, B, 32, img, dest, ref, tol_bf16(K, mag, ref),
                        "%s heads region %d" % (what, i))


def sched_ops(be, M, N):
    """Operands of the epilogues besides X and W: the residual stream, the gain, the head count."""
    rs = np.random.RandomState(M + N)
    h0 = rs.standard_normal((M, N)).astype(np.float32)
    g = (1 + 0.2 * rs.standard_normal(N)).astype(np.float32)
    H = next(h for h in (16, 10, 4, 3, 2) if N % (h * 64) == 0 and N // (h * 64) <= 3)
    return dict(h0=h0, g=g, h0_tiled=pk.tile_f32(h0), G=be.buf(g), np4=(N // 64 + 3) // 4 * 4, H=H)


def sched_epis(N):
    return [EPI_PK, EPI_HEADS] + ([EPI_RESID_NORM] if N <= GP_GAIN_MAX else [])


# (M, N, K, variant, cap).  The emulator's "CU" count is 8: a larger cap acts as 8 there.  Emulator time of a case = all its epilogues x (capped,
# uncapped where that is another grid, two-stage counterpart): 3 ... 13 s, next to 26 s for the slowest emulator case of test_kernels.py
# (test_attention_encoder_bias[1150-1280-8-2-emu]), so every one of them runs on both backends; the one GPU-only case is further down.
SCHED_CASES = [
    pytest.param(1984, 768, 128, 6, 8, id="balanced-7to8-linear-ti5"),
    pytest.param(1984, 768, 384, 6, 8, id="balanced-7to8-linear-ti5-three-laps"),
    pytest.param(1568, 768, 128, 5, 8, id="balanced-7to8-linear-ti4"),
    pytest.param(1984, 3072, 128, 6, 16, id="balanced-column-groups-only-ti5"),
    pytest.param(2592, 2048, 128, 5, 8, id="column-groups-and-leftovers-ti4"),
    pytest.param(2592, 2048, 128, 6, 8, id="column-groups-and-leftovers-ti5"),
    pytest.param(992, 1280, 128, 6, 6, id="round-robin-cap6-ti5"),
    pytest.param(992, 1280, 128, 5, 6, id="round-robin-cap6-ti4"),
]


def expect_branches(name_id, sm, hip):
    """What each case is named for (the numbers come from running pp_schedule on the host: 8 workgroups on the emulator; on the GPU the cap)."""
    M, N, K, variant, cap = name_id
    if (M, N) in ((1984, 768), (1568, 768)):
        assert sm["balanced"] and sm["tiles"] == 24 and sm["G"] == 8 and set(sm["per_wg"]) == {3} and sm["cg_tiles"] == 0 and sm["xcd"]
    elif (M, N) == (1984, 3072):
        assert sm["balanced"] and sm["tiles"] == 96 and sm["linear_tiles"] == 0 and sm["xcd"]
        assert sm["G"] == (16 if hip else 8) and set(sm["per_wg"]) == ({6} if hip else {12})
    elif (M, N) == (2592, 2048):
        assert sm["G"] == 8 and sm["cg_tiles"] > 0 and sm["linear_tiles"] > 0 and sm["short"] and sm["xcd"]
        assert 9 <= min(sm["per_wg"]) and max(sm["per_wg"]) <= 11
    elif (M, N) == (992, 1280):
        assert sm["G"] == 6 and not sm["xcd"] and sm["cg_tiles"] == 0 and set(sm["per_wg"]) <= {3, 4} and len(set(sm["per_wg"])) == 2


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("M,N,K,variant,cap", SCHED_CASES)
def test_pp_schedule_forms(be_name, M, N, K, variant, cap):
    """Ping-pong kernel with its workgroup count capped (mgk_set_pp_groups), so that a workgroup walks several tiles on the real grid as on
    the emulator: packed, per-head and (N <= 2048) tiled-residual epilogues against the reference, and the same bits as the uncapped launch
    and as the two-stage kernel of the same tile height (variant 5 against 2, 6 against 4)."""
    be = get_backend(be_name)
    TI = 4 if variant == 5 else 5
    for epi in sched_epis(N):
        sm = pp_summary(pp_schedule(M, N, K, TI, epi, ncu_of(be), cap))
        print("schedule (%d, %d, %d) TI %d cap %d epi %d: %s" % (M, N, K, TI, cap, epi, {k: v for k, v in sm.items() if k != "per_wg"}),
              "tiles per workgroup %d..%d" % (min(sm["per_wg"]), max(sm["per_wg"])))
        expect_branches((M, N, K, variant, cap), sm, be_name == "hip")
    x, w, ref, mag = problem(M, N, K)
    X, W = be.buf(pk.pack_tiles(x)), be.buf(pk.pack_tiles(w))
    ops = sched_ops(be, M, N)
    rowlive = np.ones(M, bool)
    for epi in sched_epis(N):
        res = {}
        same_grid = pp_schedule(M, N, K, TI, epi, ncu_of(be), cap) == pp_schedule(M, N, K, TI, epi, ncu_of(be), 0)
        for name, v, c in (("capped", variant, cap), ("uncapped", variant, 0), ("two-stage", 2 if variant == 5 else 4, 0)):
            if name == "uncapped" and same_grid:      # (the emulator's 8 "CUs" with a cap of 8 or more: the very same launch)
                res[name] = res["capped"]
                continue
            be.lib.mgk_gemm_set_variant(v)
            be.lib.mgk_set_pp_groups(c)
            res[name] = run_epi(be, epi, X, W, M, N, K, ops, {})
        check_epi(epi, res["capped"], M, N, K, ops, rowlive, "epi %d capped" % epi)
        for other in ("uncapped", "two-stage"):
            for key in res["capped"]:
                same_bits(res["capped"][key], res[other][key], "epi %d %s: capped against %s" % (epi, key, other))


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("variant", [5, 6])
@pytest.mark.parametrize("n_live", [1, 0])
def test_pp_schedule_one_or_no_live_tile(be_name, variant, n_live):
    """(1280, 512, 128) with a row-tile list of one tile - wave row 1 of the only block has no tile - and with an empty list: both kernels
    leave before any operand load then (gemm_xl_kernel: nblk = 0, `bid >= nblk`; gemm_pp_kernel: nbm = 0, n_my = 0) and nothing is written.
    row_tile_list never makes an empty list (a mask without an attended position gives {0}): the empty one is the test's own, count 0 and
    zeros behind it."""
    be = get_backend(be_name)
    M, N, K = 1280, 512, 128
    TI = 4 if variant == 5 else 5
    live = np.zeros(M // 32, bool)
    if n_live:
        live[17] = True
    rowlive = np.repeat(live, 32)
    for epi in sched_epis(N):
        sm = pp_summary(pp_schedule(M, N, K, TI, epi, ncu_of(be), 0, n_list=n_live))
        assert sm["tiles"] == 2 * n_live and sm["empty_row"] == bool(n_live) and not sm["balanced"]
    x, w, ref, mag = problem(M, N, K)
    X, W = be.buf(pk.pack_tiles(x)), be.buf(pk.pack_tiles(w))
    ops = sched_ops(be, M, N)
    for epi in sched_epis(N):
        res = {}
        for v in (variant, 2 if variant == 5 else 4):
            be.lib.mgk_gemm_set_variant(v)
            scratch = be.zeros((M // 32 + 1,), np.int32)
            extra = dict(row_mask=be.buf(row_mask_of(live)), list_scratch=scratch) if n_live else dict(list_scratch=scratch)
            res[v] = run_epi(be, epi, X, W, M, N, K, ops, extra)
            assert scratch.numpy()[0] == n_live
            check_epi(epi, res[v], M, N, K, ops, rowlive, "epi %d variant %d" % (epi, v))
        for key in res[variant]:
            same_bits(res[variant][key], res[2 if variant == 5 else 4][key], "epi %d %s: ping-pong against two-stage" % (epi, key))


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("variant", [5, 6])
def test_pp_schedule_eight_launches(be_name, variant):
    """(352, 512, 128) with mgk_set_pp_parts(8): 11 row tiles in 8 launches of 1 or 2 tiles each, bit-identical to one launch."""
    be = get_backend(be_name)
    M, N, K = 352, 512, 128
    TI = 4 if variant == 5 else 5
    s8 = pp_schedule(M, N, K, TI, EPI_PK, ncu_of(be), 0, parts_mode=8)
    assert s8["parts"] == 8 and sorted(set(L["nrt"] for L in s8["launches"])) == [1, 2] and sum(L["nrt"] for L in s8["launches"]) == 11
    assert pp_summary(s8)["empty_row"] and pp_schedule(M, N, K, TI, EPI_PK, ncu_of(be), 0)["parts"] == 1
    x, w, ref, mag = problem(M, N, K)
    X, W = be.buf(pk.pack_tiles(x)), be.buf(pk.pack_tiles(w))
    ops = sched_ops(be, M, N)
    be.lib.mgk_gemm_set_variant(variant)
    for epi in sched_epis(N):
        res = {}
        for mode in (0, 8):
            be.lib.mgk_set_pp_parts(mode)
            res[mode] = run_epi(be, epi, X, W, M, N, K, ops, {})
        check_epi(epi, res[8], M, N, K, ops, np.ones(M, bool), "epi %d in 8 launches" % epi)
        for key in res[0]:
            same_bits(res[0][key], res[8][key], "epi %d %s: 8 launches against one" % (epi, key))


@pytest.mark.gpu
def test_pp_schedule_full_grid_two_tiles_per_workgroup():
    """(12800, 2048, 128), EPI_PK_RELU, no cap, default variant: 320 tiles on the real grid of one workgroup per CU - the one case where an
    uncapped grid gives two tiles per workgroup and column groups together.  GPU only: the emulator has 8 "CUs" (another schedule, and more
    tiles per workgroup than the kernel's table holds), and at the 0.25 GMAC/s seen on the other cases a launch of 3.4 GMAC would take it 13 s."""
    be = get_backend("hip")
    M, N, K = 12800, 2048, 128
    ncu = ncu_of(be)
    sm = pp_summary(pp_schedule(M, N, K, 5, EPI_PK_RELU, ncu, 0))
    print("schedule:", {k: v for k, v in sm.items() if k != "per_wg"}, "tiles per workgroup %d..%d" % (min(sm["per_wg"]), max(sm["per_wg"])))
    assert sm["tiles"] == 320 and sm["cg_tiles"] > 0
    if ncu == 256:
        assert sm["G"] == 256 and max(sm["per_wg"]) == 2 and min(sm["per_wg"]) == 1
    x, w, ref, mag = problem(M, N, K)
    X, W = be.buf(pk.pack_tiles(x)), be.buf(pk.pack_tiles(w))
    res = {}
    for v in (3, 4):
        be.lib.mgk_gemm_set_variant(v)
        res[v] = run_epi(be, EPI_PK_RELU, X, W, M, N, K, None, {})
    check_epi(EPI_PK_RELU, res[3], M, N, K, None, np.ones(M, bool), "default variant")
    same_bits(res[3]["out_pk"], res[4]["out_pk"], "ping-pong against two-stage")
    problem.cache_clear()                        # (0.4 GB of float64 reference)
