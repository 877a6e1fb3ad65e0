"""Operator-level tests of the OCSR vision branch's kernels (csrc/k_swin.hip and the GEMM epilogues added for it), on the emulator and,
marked gpu, on the device - through the test entries mgk_swin_* / mgk_gemm / mgk_gemm_norm.

References are float64 numpy restatements of stock transformers `modeling_swin.py` on the bf16-rounded operands, written here from
the stock semantics (torch.roll(-shift), window_partition, relative_position_index, the -100 region mask, softmax, window_reverse,
torch.roll(+shift)).  `test_window_attention_reference_is_stock` pins the window-attention restatement to stock `SwinLayer` /
`SwinAttention`; the kernels are pinned to the restatement (the arrangement of tests/test_beam_stock.py).

Before a window-attention case launches the kernel it asserts ON THE REFERENCES ALONE that the case can see a wrong kernel: a table
index transposed, negated or one column off, a dropped key, a neighbour head's table, and for shifted windows a missing mask, a region
threshold one off and a reversed roll each move the float64 result by more than 4x the tolerance somewhere.

Tolerances are the project's for the same storage points: attention outputs stored in bf16 rtol 1/128, atol 2e-3 max|V|
(tests/test_attention_step.py); packed GEMM outputs rtol 1/128, atol 1e-3 (2e-3 behind a GELU); fp32 GEMM outputs rtol = atol = 1e-4
(tests/test_kernels.py).  The LayerNorm bound is derived from the reference's own fp32 error, see `ln_bound`."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import pkutil as pk
from tests.backends import get_backend
from tests.refutil import ln_bound, ln_ref

BACKENDS = [pytest.param("emu"), pytest.param("hip", marks=pytest.mark.gpu)]
GPU = pytest.mark.gpu
EPI_PK_BIAS, EPI_PK_GELU_ERF, EPI_RESID_NORM = 8, 9, 5
MG_E_SHAPE, MG_E_UNSUPPORTED = -1, -5
NAN_BITS = 0x7FC1                 # bf16 quiet NaN with a payload: a row the kernel fails to write shows as NaN


@pytest.fixture(autouse=True)
def _default_gemm_variant():
    """Tests that select a GEMM tile-kernel variant leave the library on its default afterwards, whatever happened in between."""
    yield
    from tests import backends as _b
    for be in _b._cache.values():
        be.lib.mgk_gemm_set_variant(3)


def _lib(be):
    L = be.lib
    L.mgk_swin_attention.argtypes = [C.c_void_p] * 4 + [C.c_int] * 6
    L.mgk_swin_layernorm.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_int] * 3 + [C.c_float, C.c_int]
    L.mgk_swin_resize.argtypes = [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_void_p] * 2
    L.mgk_swin_im2col_pack.argtypes = [C.c_void_p] * 3 + [C.c_int] * 5
    L.mgk_swin_transpose.argtypes = [C.c_void_p] * 3 + [C.c_int] * 2
    L.mgk_gemm.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.mgk_gemm_norm.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 2 + [C.c_int] * 3 + [C.c_void_p] * 4 + \
        [C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_float]
    return L


def rs(seed):
    return np.random.RandomState(seed)


def both(cases, device_only=()):
    """the cases on both backends, the device-only ones on the device alone (the emulator walks every lane of every wave on one core)"""
    return [pytest.param("emu", *c) for c in cases] + [pytest.param("hip", *c, marks=GPU) for c in list(cases) + list(device_only)]


# =====================================================================================================================================
# window attention
# =====================================================================================================================================
def rel_index(w, mut=None):
    """stock SwinRelativePositionBias._create_relative_position_index ([query][key] -> row of the table); `mut` states a wrong kernel."""
    coords = np.stack(np.meshgrid(np.arange(w), np.arange(w), indexing="ij")).reshape(2, -1)
    rel = coords[:, :, None] - coords[:, None, :]                    # [2][n][n]: query - key
    if mut == "negate":
        rel = -rel
    if mut == "transpose":
        rel = rel[::-1]
    rel = rel.transpose(1, 2, 0).copy()
    rel[:, :, 0] += w - 1
    rel[:, :, 1] += w - 1
    rel[:, :, 0] *= 2 * w - 1
    idx = rel.sum(-1)
    if mut == "col_off":
        idx = np.minimum(idx + 1, (2 * w - 1) ** 2 - 1)
    return idx


def window_partition(x, w):
    B, Hh, Ww, Cc = x.shape
    return x.reshape(B, Hh // w, w, Ww // w, w, Cc).transpose(0, 1, 3, 2, 4, 5).reshape(-1, w, w, Cc)


def window_reverse(win, w, Hh, Ww):
    Cc = win.shape[-1]
    return win.reshape(-1, Hh // w, Ww // w, w, w, Cc).transpose(0, 1, 3, 2, 4, 5).reshape(-1, Hh, Ww, Cc)


def shift_mask(R, w, shift, thr_off=0):
    """stock SwinLayer.get_attn_mask: the map is cut by the slices (0, -w), (-w, -shift), (-shift, None) on each axis, region id =
    3 * row part + column part, -100 where the ids of query and key differ.  thr_off = 1: the second cut one position late."""
    img = np.zeros((1, R, R, 1))
    if thr_off == 0:
        cnt = 0
        for hs in (slice(0, -w), slice(-w, -shift), slice(-shift, None)):
            for ws in (slice(0, -w), slice(-w, -shift), slice(-shift, None)):
                img[:, hs, ws, :] = cnt
                cnt += 1
    else:
        a = np.arange(R)
        reg = (a >= R - w).astype(int) + (a > R - shift).astype(int)
        img[0, :, :, 0] = reg[:, None] * 3 + reg[None, :]
    mw = window_partition(img, w).reshape(-1, w * w)
    d = mw[:, None, :] - mw[:, :, None]
    return np.where(d != 0, -100.0, 0.0)                              # [windows][n][n]


def swin_attention_ref(q, k, v, table, B, R, H, w, shift, mut=None):
    """q, k, v float64 [B*R*R][H*32] (natural token order), table [(2w-1)^2][H] as stock stores it -> context [B*R*R][H*32]."""
    n, Cc = w * w, H * 32
    s = shift if mut != "roll_rev" else -shift

    def windows(x):
        x = x.reshape(B, R, R, Cc)
        if shift:
            x = np.roll(x, (-s, -s), axis=(1, 2))
        return window_partition(x, w).reshape(-1, n, H, 32).transpose(0, 2, 1, 3)          # [B*nW][H][n][32]
    qw, kw, vw = windows(q), windows(k), windows(v)
    sc = np.einsum("whqd,whkd->whqk", qw, kw) * (32 ** -0.5)
    tab = table if mut != "head_swap" else np.roll(table, -1, axis=1)
    sc = sc + tab[rel_index(w, mut).reshape(-1)].reshape(n, n, H).transpose(2, 0, 1)[None]
    if shift and mut != "no_mask":
        m = shift_mask(R, w, shift, 1 if mut == "thresh" else 0)
        sc = (sc.reshape(B, -1, H, n, n) + m[None, :, None]).reshape(-1, H, n, n)
    if mut == "drop_key":
        sc[..., n - 1] = -np.inf
    sc = sc - sc.max(-1, keepdims=True)
    p = np.exp(sc)
    p /= p.sum(-1, keepdims=True)
    ctx = np.einsum("whqk,whkd->wqhd", p, vw).reshape(-1, w, w, Cc)
    out = window_reverse(ctx, w, R, R)
    if shift:
        out = np.roll(out, (s, s), axis=(1, 2))
    return out.reshape(B * R * R, Cc)


def attention_inputs(B, R, H, w, seed):
    """q, k ~ 1.5 N(0,1), v ~ N(0,1), table ~ U(-3,3), bf16-rounded; every head and image its own values."""
    r = rs(seed)
    M, Cc = B * R * R, H * 32
    q = pk.bf16_round(1.5 * r.standard_normal((M, Cc))).astype(np.float64)
    k = pk.bf16_round(1.5 * r.standard_normal((M, Cc))).astype(np.float64)
    v = pk.bf16_round(r.standard_normal((M, Cc))).astype(np.float64)
    table = pk.bf16_round(r.uniform(-3, 3, ((2 * w - 1) ** 2, H))).astype(np.float64)
    return q, k, v, table


def assert_case_sees_mutants(q, k, v, table, B, R, H, w, shift, ref, atol, rtol):
    muts = ["transpose", "negate", "col_off", "drop_key"] + (["head_swap"] if H > 1 else []) + \
           (["no_mask", "thresh", "roll_rev"] if shift else [])
    for mu in muts:
        bad = swin_attention_ref(q, k, v, table, B, R, H, w, shift, mut=mu)
        ratio = (np.abs(bad - ref) / (atol + rtol * np.abs(ref))).max()
        assert ratio > 4.0, (mu, ratio)


# (w, R, shift, H, B): w in {4, 8, 12}; R in {w, 2w, 3w} (and 4w for w = 4: 3w has an interior window without a masked pair beside
# eight boundary windows of three mask patterns); shift 0 and w / 2 where R > w, one odd shift; H = 1, 2, 3 (fewer heads than waves),
# 4, 8 (two head groups per window); B = 1, 2, 3 (R = 4, B = 3: 48 rows are not a whole 32-row tile).  The emulator walks every lane of
# every wave: w = 12 stays at one image, up to 9 windows and 4 heads there; the Swin-B stage geometries run on the device only.
ATT_CASES = [
    (4, 4, 0, 1, 3), (4, 4, 0, 8, 1), (4, 8, 0, 2, 2), (4, 8, 2, 3, 1), (4, 12, 0, 4, 1), (4, 12, 2, 8, 2), (4, 16, 2, 4, 1),
    (4, 16, 0, 3, 1), (4, 8, 2, 1, 3),
    (8, 8, 0, 2, 1), (8, 8, 0, 8, 2), (8, 16, 0, 1, 1), (8, 16, 4, 4, 2), (8, 24, 4, 2, 1), (8, 24, 0, 3, 1), (8, 16, 3, 3, 1),
    (8, 24, 4, 8, 1), (8, 16, 4, 1, 3),
    (12, 12, 0, 4, 1), (12, 12, 0, 1, 1), (12, 24, 0, 2, 1), (12, 24, 6, 3, 1), (12, 36, 6, 4, 1), (12, 36, 0, 1, 1),
]
ATT_DEVICE = [(12, 96, 6, 4, 2), (12, 48, 6, 8, 2), (12, 24, 6, 16, 2), (12, 12, 0, 32, 2),       # the Swin-B stages at two images
              (8, 24, 4, 32, 1), (4, 8, 2, 32, 3), (12, 36, 6, 8, 3), (12, 24, 0, 2, 3)]


@pytest.mark.parametrize("be_name,w,R,shift,H,B", both(ATT_CASES, ATT_DEVICE))
def test_window_attention(be_name, w, R, shift, H, B):
    be = get_backend(be_name)
    L = _lib(be)
    M, Cc = B * R * R, H * 32
    Mp = (M + 31) // 32 * 32
    q, k, v, table = attention_inputs(B, R, H, w, 1000 + 97 * w + 13 * R + 5 * shift + H + 31 * B)
    ref = swin_attention_ref(q, k, v, table, B, R, H, w, shift)
    rtol, atol = 1.0 / 128, 2e-3 * np.abs(v).max()
    if M * Cc <= 3 * 36 * 36 * 256:      # (the mutant references of the largest device geometries would take minutes on the host)
        assert_case_sees_mutants(q, k, v, table, B, R, H, w, shift, ref, atol, rtol)
    qkv = be.buf(pk.pack_tiles(np.concatenate([q, k, v], axis=1).astype(np.float32)))
    ctx = be.buf(np.full((Mp * Cc,), NAN_BITS, np.uint16))
    tab = be.buf(np.ascontiguousarray(table.T).astype(np.float32))                        # [H][(2w-1)^2]
    assert L.mgk_swin_attention(be.stream, be.p(qkv), be.p(ctx), be.p(tab), B, R, Cc, H, w, shift) == 0
    bits = pk.unpack_tile_bits(ctx.numpy(), Cc)
    assert (bits[M:] == NAN_BITS).all()                                                    # padding rows are not written
    got = pk.bf16_to_f32(bits[:M])
    assert np.isfinite(got).all()                                                          # every row < M was written
    print(f"w={w} R={R} shift={shift} H={H} B={B}: max err / tol = {(np.abs(got - ref) / (atol + rtol * np.abs(ref))).max():.3f}")
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=atol)


def test_entries_reject_what_the_launchers_assume():
    be = get_backend("emu")
    L = _lib(be)
    d = be.zeros((64,), np.float32)
    p = be.p(d)
    assert L.mgk_swin_attention(be.stream, p, p, p, 1, 8, 64, 2, 6, 0) == MG_E_UNSUPPORTED     # window 6
    assert L.mgk_swin_attention(be.stream, p, p, p, 1, 10, 64, 2, 4, 0) == MG_E_UNSUPPORTED    # a map that is not whole windows
    assert L.mgk_swin_attention(be.stream, p, p, p, 1, 8, 64, 4, 4, 0) == MG_E_UNSUPPORTED     # head dim 16
    assert L.mgk_swin_attention(be.stream, p, p, p, 1, 8, 192, 6, 4, 0) == MG_E_UNSUPPORTED    # 6 heads: not whole groups of 4
    assert L.mgk_swin_attention(be.stream, p, p, p, 1, 8, 64, 2, 4, 4) == MG_E_SHAPE           # shift >= w
    assert L.mgk_swin_attention(be.stream, p, p, p, 1, 8, 64, 2, 4, -1) == MG_E_SHAPE
    assert L.mgk_swin_layernorm(be.stream, p, 0, None, 0, p, p, None, None, p, 1, 96, 0, 1e-5, 0) == MG_E_UNSUPPORTED   # no case for 96
    assert L.mgk_swin_layernorm(be.stream, p, 1, None, 0, p, p, None, None, p, 1, 256, 3, 1e-5, 0) == MG_E_SHAPE        # odd merge_R
    assert L.mgk_swin_layernorm(be.stream, p, 0, None, 0, p, p, None, p, None, 1, 64, 0, 1e-5, 72) == MG_E_SHAPE        # kaug % 16
    assert L.mgk_swin_layernorm(be.stream, p, 0, None, 0, p, p, None, p, None, 1, 64, 0, 1e-5, 48) == MG_E_SHAPE        # kaug < C
    assert L.mgk_gemm(be.stream, 1, EPI_PK_BIAS, p, p, 32, 64, 64, None, 0, None, p) == MG_E_UNSUPPORTED               # mode 0 only
    assert L.mgk_gemm(be.stream, 0, 10, p, p, 32, 64, 64, None, 0, None, p) == MG_E_SHAPE


@pytest.mark.parametrize("w", [4, 8, 12])
@pytest.mark.parametrize("nwin,half", [(1, False), (2, False), (2, True), (3, True)])
def test_window_attention_reference_is_stock(w, nwin, half):
    """The float64 restatement above against stock transformers: SwinLayer's own cyclic_shift / get_attn_mask / SwinAttention /
    window_partition / window_reverse in float64, with random q / k / v projections and an identity output projection."""
    import torch
    from transformers import SwinConfig
    from transformers.models.swin import modeling_swin as ms
    R, shift, H, B = nwin * w, (w // 2 if half else 0), 2, 2
    Cc = 32 * H
    cfg = SwinConfig(window_size=w, qkv_bias=True)
    cfg._attn_implementation = "eager"
    layer = ms.SwinLayer(cfg, Cc, (R, R), H, shift_size=shift).double().eval()
    r = rs(7 + w + nwin)
    att = layer.attention
    with torch.no_grad():
        for lin in (att.q_proj, att.k_proj, att.v_proj):
            lin.weight.copy_(torch.from_numpy(r.standard_normal((Cc, Cc)) / math.sqrt(Cc) * 1.5))
            lin.bias.copy_(torch.from_numpy(r.standard_normal(Cc) * 0.1))
        att.o_proj.weight.copy_(torch.eye(Cc, dtype=torch.float64))
        att.o_proj.bias.zero_()
        att.relative_position_bias.relative_position_bias_table.copy_(torch.from_numpy(r.uniform(-3, 3, ((2 * w - 1) ** 2, H))))
        x = torch.from_numpy(r.standard_normal((B, R, R, Cc)))
        win = ms.window_partition(layer.cyclic_shift(x), w).view(-1, w * w, Cc)
        mask = layer.get_attn_mask(R, R, dtype=x.dtype, device=x.device)
        assert (mask is None) == (shift == 0)
        o, _ = att(win, mask)
        stock = layer.cyclic_shift(ms.window_reverse(o.view(-1, w, w, Cc), w, R, R), reverse=True).reshape(B * R * R, Cc).numpy()
        xf = x.reshape(-1, Cc)
        q, k, v = (lin(xf).numpy() for lin in (att.q_proj, att.k_proj, att.v_proj))
        table = att.relative_position_bias.relative_position_bias_table.numpy()
    mine = swin_attention_ref(q, k, v, table, B, R, H, w, shift)
    assert np.abs(mine - stock).max() < 1e-5
    if shift:                        # the explicit slices above state the same mask as stock's arithmetic form
        assert np.array_equal(shift_mask(R, w, shift), mask.numpy())


# =====================================================================================================================================
# LayerNorm / patch merging
# =====================================================================================================================================
def ln_params(Cc, seed):
    r = rs(seed)
    return (1 + 0.3 * r.standard_normal(Cc)).astype(np.float32), (0.3 * r.standard_normal(Cc)).astype(np.float32), \
        r.standard_normal(Cc).astype(np.float32)


def run_ln(be, x_src, in_tiled, M, Cc, w, b, eps, add_bias=None, want=("f32", "pk", "h"), h_norm=0, kaug=0, in_place=False, merge_R=0):
    """launch mgk_swin_layernorm; returns the outputs WITH their padding rows"""
    L = _lib(be)
    Mp = (M + 31) // 32 * 32
    hin = be.buf(x_src)
    outs = {}
    f32 = be.buf(np.full((M, Cc), np.nan, np.float32)) if "f32" in want else None
    kw = kaug if kaug else Cc
    xpk = be.buf(np.full((Mp * kw,), NAN_BITS, np.uint16)) if "pk" in want else None
    hout = None
    if "h" in want:
        hout = hin if in_place else be.buf(np.full((Mp * Cc,), -77.0, np.float32))
    ab = be.buf(add_bias) if add_bias is not None else None
    rc = L.mgk_swin_layernorm(be.stream, be.p(hin), in_tiled, be.p(hout), h_norm, be.p(be.buf(w)), be.p(be.buf(b)), be.p(ab), be.p(xpk),
                              be.p(f32), M, Cc, merge_R, eps, kaug)
    assert rc == 0
    if f32 is not None:
        outs["f32"] = f32.numpy().copy()
    if xpk is not None:
        outs["pk"] = pk.unpack_tile_bits(xpk.numpy(), kw)
    if hout is not None:
        outs["h"] = pk.untile_f32(hout.numpy(), Cc)
    return outs


def check_ln_outputs(outs, x, ref, bound, M, Cc, add_bias, h_norm, kaug=0, in_place=False, label=None):
    if "f32" in outs:
        err = np.abs(outs["f32"] - ref)
        if label:
            print(f"{label} out_f32: max err {err.max():.3e}, bound {bound.min():.3e} .. {bound.max():.3e}, max err / bound {(err / np.maximum(bound, 1e-300)).max():.3f}")
        assert (err <= bound).all(), (err / np.maximum(bound, 1e-300)).max()
    if "pk" in outs:
        bits = outs["pk"]
        assert (bits[M:] == NAN_BITS).all()
        got = pk.bf16_to_f32(bits[:M, :Cc])
        assert (np.abs(got - ref) <= bound + 2.0 ** -8 * np.abs(ref)).all()
        if kaug:
            assert (bits[:M, Cc] == 0x3F80).all() and (bits[:M, Cc + 1:] == 0).all()
    if "h" in outs:
        h = outs["h"]
        assert (h[M:] == (-55.0 if in_place else -77.0)).all()
        if h_norm:
            want = ref + (add_bias.astype(np.float64) if add_bias is not None else 0.0)
            assert (np.abs(h[:M] - want) <= bound + 2.0 ** -23 * np.abs(want)).all()
        else:
            want = np.float32(x) + (np.float32(add_bias) if add_bias is not None else np.float32(0))
            assert np.array_equal(h[:M].view(np.uint32), want.astype(np.float32).view(np.uint32))


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("M", [1, 31, 32, 33, 70])
@pytest.mark.parametrize("Cc", [64, 128, 256, 512, 768, 1024, 2048, 4096])
def test_layernorm_every_width_and_form(be_name, Cc, M):
    """Every width the launcher has a case for (values kept in registers up to 1024, three passes from 2048 on) x row counts around the
    32-row tile (partial last tile, the row clamp of inactive lanes) x the forms the branch and the ChemicalOCR tower launch: row-major
    and tiled input, in place, add_bias null and given, each output alone and all together, normalised h_out, the constant-one column.
    Measured on these inputs: float32 restatement against float64 3.1e-7 .. 1.05e-6 (largest per case), bound (8x) 2.5e-6 .. 8.4e-6; the
    kernel's largest error is 0.25 of the bound on an MI355X."""
    be = get_backend(be_name)
    eps = 1e-5
    r = rs(50 + Cc + M)
    x = ((0.5 + r.uniform(0, 2, (M, 1))) * r.standard_normal((M, Cc)) + r.standard_normal((M, 1))).astype(np.float32)
    w, b, ab = ln_params(Cc, Cc + 3 * M)
    ref, bound = ln_bound(x, w, b, eps)
    tiled = pk.tile_f32(x, pad_value=-55.0)
    # row-major input, everything at once, add_bias given
    o = run_ln(be, x, 0, M, Cc, w, b, eps, add_bias=ab)
    check_ln_outputs(o, x, ref, bound, M, Cc, ab, 0, label=f"C={Cc} M={M}")
    # tiled input, in place (what every block's LN1 / LN2 does), add_bias given, packed output
    o = run_ln(be, tiled, 1, M, Cc, w, b, eps, add_bias=ab, want=("pk", "h"), in_place=True)
    check_ln_outputs(o, x, ref, bound, M, Cc, ab, 0, in_place=True)
    # tiled input, in place without add_bias: the rows come back bit-equal
    o = run_ln(be, tiled, 1, M, Cc, w, b, eps, want=("h",), in_place=True)
    check_ln_outputs(o, x, ref, bound, M, Cc, None, 0, in_place=True)
    # each output alone
    check_ln_outputs(run_ln(be, tiled, 1, M, Cc, w, b, eps, want=("f32",)), x, ref, bound, M, Cc, None, 0)
    check_ln_outputs(run_ln(be, x, 0, M, Cc, w, b, eps, want=("pk",)), x, ref, bound, M, Cc, None, 0)
    # normalised h_out (embeddings.norm: its output is the residual stream), without and with add_bias
    check_ln_outputs(run_ln(be, x, 0, M, Cc, w, b, eps, want=("h",), h_norm=1), x, ref, bound, M, Cc, None, 1)
    check_ln_outputs(run_ln(be, tiled, 1, M, Cc, w, b, eps, add_bias=ab, want=("h", "f32"), h_norm=1), x, ref, bound, M, Cc, ab, 1)
    # bias-in-K column of the ChemicalOCR tower's projections
    check_ln_outputs(run_ln(be, x, 0, M, Cc, w, b, eps, want=("pk",), kaug=Cc + 64), x, ref, bound, M, Cc, None, 0, kaug=Cc + 64)


def merge_gather(hmap, B, R, Cin, swapped=False):
    """stock SwinPatchMerging: [x[0::2, 0::2] | x[1::2, 0::2] | x[0::2, 1::2] | x[1::2, 1::2]] on the feature axis"""
    m = hmap.reshape(B, R, R, Cin)
    parts = [m[:, 0::2, 0::2], m[:, 1::2, 0::2], m[:, 0::2, 1::2], m[:, 1::2, 1::2]]
    if swapped:
        parts = [parts[0], parts[2], parts[1], parts[3]]
    return np.concatenate(parts, -1).reshape(B * (R // 2) ** 2, 4 * Cin)


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("Cin", [64, 128, 512, 1024])
@pytest.mark.parametrize("R", [2, 4, 8, 24])
def test_layernorm_patch_merging_gather(be_name, R, Cin, B):
    """merge_R: the 2 x 2 gather in stock's order in front of LayerNorm(4 Cin) (4 Cin = 2048, 4096: the three-pass form re-reads the
    gather), every output; every (b, y, x) of the map holds values of its own, and the case is shown to tell stock's order from
    the row / column swapped one on the references alone."""
    be = get_backend(be_name)
    Cc, M, eps = 4 * Cin, B * (R // 2) ** 2, 1e-5
    r = rs(R * 1000 + Cin + B)
    hmap = (r.standard_normal((B * R * R, Cin)) + r.standard_normal((B * R * R, 1))).astype(np.float32)
    w, b, _ = ln_params(Cc, 9 + Cin)
    x = merge_gather(hmap, B, R, Cin)
    ref, bound = ln_bound(x, w, b, eps)
    wrong = ln_ref(merge_gather(hmap, B, R, Cin, swapped=True), w, b, eps)
    assert (np.abs(wrong - ref) / bound).max() > 4
    o = run_ln(be, pk.tile_f32(hmap), 1, M, Cc, w, b, eps, merge_R=R)
    check_ln_outputs(o, x, ref, bound, M, Cc, None, 0, label=f"merge R={R} Cin={Cin} B={B}")


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("Cc", [64, 256, 768, 1024, 2048, 4096])
def test_layernorm_rows_that_break_a_careless_kernel(be_name, Cc):
    """Rows of mean 100 and deviation 0.05 (a one-pass E[x^2] - mean^2 variance in float32 fails on them: asserted on the references
    alone), a constant row (variance 0: the output is b, finite) and a row of magnitude 1e4 between rows of order 1 in the same 32-row
    tile (the rows of a tile share a workgroup and its reduction buffer: they must not mix).  The bound is taken per kind of row.
    Measured: float32 restatement on the mean-100 rows 7.7e-5 .. 3.0e-4 by width (the mean's rounding divided by the deviation), bound
    6.2e-4 .. 2.4e-3, kernel 6.4e-5 .. 4.4e-4 (at most 0.51 of the bound, width 1024); the 1e4 row: bound 1.1e-6 .. 4.5e-6, kernel < 3.9e-7."""
    be = get_backend(be_name)
    M, eps = 40, 1e-5
    r = rs(300 + Cc)
    x = r.standard_normal((M, Cc)).astype(np.float32)
    x[5] = (1e4 * r.standard_normal(Cc)).astype(np.float32)
    x[7] = 3.0
    x[10:14] = (100 + 0.05 * r.standard_normal((4, Cc))).astype(np.float32)
    x[35] = (100 + 0.05 * r.standard_normal(Cc)).astype(np.float32)
    w, b, ab = ln_params(Cc, 17 + Cc)
    kinds = np.zeros(M, int)
    kinds[5], kinds[7], kinds[10:14], kinds[35] = 1, 2, 3, 3
    ref, bound = ln_bound(x, w, b, eps, kinds)
    x32 = x[10:14]
    m1 = x32.mean(-1, keepdims=True, dtype=np.float32)
    v1 = (x32 * x32).mean(-1, keepdims=True, dtype=np.float32) - m1 * m1
    with np.errstate(invalid="ignore", divide="ignore"):
        one_pass = (x32 - m1) / np.sqrt(v1 + np.float32(eps)) * w + b
    assert not (np.abs(one_pass - ref[10:14]) <= 4 * bound[10:14]).all()
    assert np.array_equal(ref[7], b.astype(np.float64)) and bound[7, 0] == 0      # (3.0 sums exactly in any order: the kernel returns b itself)
    for tiled in (0, 1):
        o = run_ln(be, pk.tile_f32(x) if tiled else x, tiled, M, Cc, w, b, eps, add_bias=ab)
        assert np.isfinite(o["f32"]).all()
        err = np.abs(o["f32"] - ref)
        print(f"hard rows C={Cc} tiled={tiled}: mean-100 rows max err {err[10:14].max():.3e} (bound {bound[10:14].min():.3e} .. "
              f"{bound[10:14].max():.3e}), 1e4 row {err[5].max():.3e} (bound {bound[5, 0]:.3e})")
        check_ln_outputs(o, x, ref, bound, M, Cc, ab, 0, label=f"hard rows C={Cc} tiled={tiled}")
        assert np.array_equal(o["f32"][7], b)


# =====================================================================================================================================
# GEMM epilogues of the branch
# =====================================================================================================================================
def erf64(x):
    try:
        from scipy.special import erf
        return erf(np.asarray(x, np.float64))
    except ImportError:
        import torch
        return torch.erf(torch.from_numpy(np.asarray(x, np.float64))).numpy()


def gelu_exact(x):
    x = np.asarray(x, np.float64)
    return 0.5 * x * (1.0 + erf64(x / math.sqrt(2.0)))


# (variant, M, N, K, kernel the shape is meant to reach).  M is never a multiple of 32, N is a multiple of 32 that is not a multiple of
# the tile width.  Variant 3 is the default: gemm() sends problems of fewer than 256 tiles of 320 x 256 to the 256 x 128 kernel and,
# with fewer than 96 of those tiles (or M < 256), to the 128 x 128 kernel.
GEMM_CASES = [
    (0, 150, 224, 128, "128x128 two-stage"),
    (1, 300, 224, 64, "256x128 three-stage (M >= 256)"),
    (2, 340, 288, 128, "256x256 (launch_xl<., 4>)"),
    (4, 340, 288, 128, "320x256 (launch_xl<., 5>)"),
    (5, 700, 288, 128, "ping-pong, 256-row tiles"),
    (6, 700, 288, 128, "ping-pong, 320-row tiles"),
    (3, 144, 352, 128, "default, 2 tiles of 320 x 256 and M < 256: 128x128 (the last Swin stage at one image)"),
    (3, 300, 480, 64, "default, 2 x 2 tiles of 320 x 256, 2 x 4 of 256 x 128 (< 96): 128x128"),
    (3, 1100, 2528, 64, "default, 4 x 10 tiles of 320 x 256 (< 256), 5 x 20 of 256 x 128 (>= 96): 256x128"),
]
# the device tier: shapes the branch issues.  The ping-pong kernel under the default rule needs >= 256 tiles of 320 x 256 (2.7 G
# multiply-adds at the least): on the emulator that kernel is reached through variants 5 / 6 above, the rule itself here.
GEMM_DEVICE = [
    (3, 144, 3072, 1024, "last Swin-B stage QKV at one image: 128x128"),
    (3, 288, 4096, 1024, "last Swin-B stage fc1 at two images: 2 x 32 tiles of 256 x 128 (< 96): 128x128"),
    (3, 18432, 384, 128, "stage 0 QKV at two images: 58 x 2 tiles of 320 x 256, 72 x 3 of 256 x 128 -> 256x128"),
    (3, 46080, 512, 128, "stage 0 fc1 at five images: 144 x 2 = 288 tiles -> ping-pong"),
]


@pytest.mark.parametrize("be_name,variant,M,N,K,reaches", both(GEMM_CASES, GEMM_DEVICE))
def test_gemm_bias_and_gelu_erf_epilogues(be_name, variant, M, N, K, reaches):
    """EPI_PK_BIAS (8) and EPI_PK_GELU_ERF (9), bias given and null, in every tile-kernel family and on both sides of the
    small-problem rule; the bias is shown to be visible feature by feature (shifted by one float4 group it misses the tolerance 4x)."""
    be = get_backend(be_name)
    L = _lib(be)
    r = rs(variant * 7 + M + N)
    x = pk.bf16_round(r.standard_normal((M, K)))
    w = pk.bf16_round(r.standard_normal((N, K)) * (1.5 / math.sqrt(K)))
    bias = r.standard_normal(N).astype(np.float32)
    acc = x.astype(np.float64) @ w.astype(np.float64).T
    rtol = 1.0 / 128
    epis = ((EPI_PK_BIAS, 1e-3, lambda t: t), (EPI_PK_GELU_ERF, 2e-3, gelu_exact))
    for epi, atol, f in epis:
        ref = f(acc + bias)
        shifted = f(acc + np.roll(bias, 4))
        assert (np.abs(shifted - ref) / (atol + rtol * np.abs(ref))).max() > 4
    X, W = be.buf(pk.pack_tiles(x)), be.buf(pk.pack_tiles(w))
    bb = be.buf(bias)
    Mp = (M + 31) // 32 * 32
    L.mgk_gemm_set_variant(variant)
    try:
        for epi, atol, f in epis:
            for bvec, bbuf in ((bias, bb), (None, None)):
                out = be.buf(np.full((Mp * N,), NAN_BITS, np.uint16))
                assert L.mgk_gemm(be.stream, 0, epi, be.p(X), be.p(W), M, N, K, None, 0, be.p(bbuf), be.p(out)) == 0
                bits = pk.unpack_tile_bits(out.numpy(), N)
                assert (bits[M:] == NAN_BITS).all()
                ref = f(acc + bvec) if bvec is not None else f(acc)
                np.testing.assert_allclose(pk.bf16_to_f32(bits[:M]), ref, rtol=rtol, atol=atol)
    finally:
        L.mgk_gemm_set_variant(3)


@pytest.mark.parametrize("be_name", BACKENDS)
def test_gelu_erf_over_every_bf16_pre_activation(be_name):
    """gelu_erf itself (Abramowitz & Stegun 7.1.26 on fast_exp) against exact erf-GELU: X = one-hot rows, so that the pre-activation of
    (m, n) is exactly the bf16 value W[n][m]; every bf16 value of [-8, -2^-10] and [2^-10, 8] and both zeros.  Allowed: one bf16 ulp of
    the exact value plus 1e-6 (the A&S bound 1.5e-7 on erf times |x| / 2 <= 4, the exponential on top).  The negative tail returns
    neither positive values nor NaN; gelu(+-0) = 0.  Once more with a bias (pre-activation = bf16 value + bias, rounded to fp32).
    Measured (emulator and MI355X alike): the largest excess over one ulp is 7.6e-8, at x = -5.53 where the exact value is -8.8e-8."""
    be = get_backend(be_name)
    L = _lib(be)
    mags = np.arange(0x3A80, 0x4100 + 1, dtype=np.uint16)                      # 2^-10 .. 8.0
    vals = np.concatenate([mags, mags | 0x8000, np.array([0x0000, 0x8000], np.uint16)])
    M = K = 64
    N = (vals.size + 63) // 64
    N = (N + 31) // 32 * 32
    wbits = np.zeros(N * K, np.uint16)
    wbits[:vals.size] = vals
    w = pk.bf16_to_f32(wbits).reshape(N, K)
    assert np.abs(w).max() == 8.0 and np.abs(w[w != 0]).min() == 2.0 ** -10
    x = np.eye(M, K, dtype=np.float32)
    X, W = be.buf(pk.pack_tiles(x)), be.buf(pk.pack_tiles(w))
    bias = pk.bf16_round(rs(5).uniform(-1, 1, N)).astype(np.float32)
    for bvec in (None, bias):
        out = be.buf(np.full((M * N,), NAN_BITS, np.uint16))
        bbuf = be.buf(bvec) if bvec is not None else None
        assert L.mgk_gemm(be.stream, 0, EPI_PK_GELU_ERF, be.p(X), be.p(W), M, N, K, None, 0, be.p(bbuf), be.p(out)) == 0
        got = pk.unpack_tiles(out.numpy(), M, N).astype(np.float64)           # [m][n]: pre-activation w[n][m] (+ bias[n])
        pre = w.T.astype(np.float32) + (bvec[None, :] if bvec is not None else np.float32(0))
        pre = pre.astype(np.float64)
        exact = gelu_exact(pre)
        want = pk.bf16_round(exact).astype(np.float64)
        ulp = np.where(exact != 0, 2.0 ** (np.floor(np.log2(np.maximum(np.abs(exact), 1e-300))) - 7), 0.0)
        err = np.abs(got - want)
        i = np.unravel_index(np.argmax(err - ulp), err.shape)
        print(f"gelu_erf bias={bvec is not None}: worst (err - ulp) {err[i] - ulp[i]:.3e} at x = {pre[i]!r} (exact {exact[i]!r}, got {got[i]!r})")
        assert np.isfinite(got).all()
        assert (err <= ulp + 1e-6).all(), (pre[i], exact[i], got[i])
        assert (got[pre < 0] <= 0).all()
        assert (got[pre == 0] == 0).all() and (pre == 0).sum() >= (2 if bvec is None else 0)


@pytest.mark.parametrize("be_name,M,N,K", both([(512, 64, 64), (144, 1024, 256), (300, 128, 128)], [(144, 1024, 4096)]))
def test_gemm_tiled_residual_without_norm_outputs(be_name, M, N, K):
    """EPI_RESID_NORM as the branch issues it (o_proj, fc2): h_tiled += X W^T with gain, partial sums and packed output all null, in the
    kernels the small-problem rule picks; rows beyond M keep their values."""
    be = get_backend(be_name)
    L = _lib(be)
    r = rs(M + N + K)
    x = pk.bf16_round(r.standard_normal((M, K)))
    w = pk.bf16_round(r.standard_normal((N, K)) / math.sqrt(K))
    h0 = r.standard_normal((M, N)).astype(np.float32)
    ref = h0.astype(np.float64) + x.astype(np.float64) @ w.astype(np.float64).T
    h = be.buf(pk.tile_f32(h0, pad_value=-55.0))
    assert L.mgk_gemm_norm(be.stream, EPI_RESID_NORM, be.p(be.buf(pk.pack_tiles(x))), be.p(be.buf(pk.pack_tiles(w))), M, N, K, be.p(h),
                           None, None, None, 0, None, 0, 0.0, 0.0) == 0
    got = pk.untile_f32(h.numpy(), N)
    assert (got[M:] == -55.0).all()
    np.testing.assert_allclose(got[:M], ref, rtol=1e-4, atol=1e-4)


# =====================================================================================================================================
# resize, im2col, transpose
# =====================================================================================================================================
RESIZE_CB = [(1, 2), (3, 1), (4, 2)]


@pytest.mark.parametrize("be_name,S,I,Cn,B", both([(S, I, c, b) for S, I in [(80, 64), (64, 64), (48, 64), (100, 64), (7, 64), (1, 8)]
                                                   for c, b in RESIZE_CB], [(1024, 384, c, b) for c, b in RESIZE_CB]))
def test_resize_is_torch_bilinear(be_name, S, I, Cn, B):
    """swin_resize against torch interpolate(bilinear, align_corners=False, antialias=False) in float32, then the affine in float64.
    Tolerance 1e-5 max|src| max|scale|: four fp32 products and three sums, weights by the same fp32 formula.  Where the sizes differ,
    align_corners=True is shown (from torch alone) to miss that by more than 100x."""
    import torch
    import torch.nn.functional as F
    be = get_backend(be_name)
    L = _lib(be)
    r = rs(S + I + Cn)
    yy, xx = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    src = np.stack([[np.sin(0.11 * (c + 1) * xx + b) * np.cos(0.07 * (b + 1) * yy + c) + 0.3 * r.standard_normal((S, S)) for c in range(Cn)]
                    for b in range(B)]).astype(np.float32)
    scale = np.array([2.18, -1.3, 0.75, 1.9][:Cn], np.float32)
    shift = np.array([0.07, -0.4, 1.5, -2.0][:Cn], np.float32)
    t = torch.from_numpy(src)
    ip = F.interpolate(t, size=(I, I), mode="bilinear", align_corners=False, antialias=False).numpy()
    ref = ip.astype(np.float64) * scale.astype(np.float64)[None, :, None, None] + shift.astype(np.float64)[None, :, None, None]
    tol = 1e-5 * np.abs(src).max() * np.abs(scale).max()
    if S != I and S > 1:
        ac = F.interpolate(t, size=(I, I), mode="bilinear", align_corners=True).numpy()
        acr = ac.astype(np.float64) * scale.astype(np.float64)[None, :, None, None] + shift.astype(np.float64)[None, :, None, None]
        assert np.abs(acr - ref).max() > 100 * tol
    dst = be.buf(np.full((B, Cn, I, I), np.nan, np.float32))
    sc_h, sh_h = np.ascontiguousarray(scale), np.ascontiguousarray(shift)
    assert L.mgk_swin_resize(be.stream, be.p(be.buf(src)), be.p(dst), B, Cn, S, I, sc_h.ctypes.data, sh_h.ctypes.data) == 0
    got = dst.numpy()
    print(f"resize S={S} I={I}: max err {np.abs(got - ref).max():.3e} (tol {tol:.3e})")
    assert np.abs(got - ref).max() <= tol


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("Cn,ps,I,B", [(3, 4, 64, 2), (1, 4, 16, 3), (3, 4, 96, 1), (4, 2, 8, 1)])
def test_swin_im2col_pack(be_name, Cn, ps, I, B):
    """bit-equal to pack_tiles of the numpy im2col, k = (c * ps + dy) * ps + dx; the columns from C ps ps on and the rows from M on are zero"""
    be = get_backend(be_name)
    L = _lib(be)
    pix = rs(Cn * 100 + I).standard_normal((B, Cn, I, I)).astype(np.float32)
    g = I // ps
    M, Kr = B * g * g, Cn * ps * ps
    Kp = (Kr + 63) // 64 * 64
    cols = pix.reshape(B, Cn, g, ps, g, ps).transpose(0, 2, 4, 1, 3, 5).reshape(M, Kr)
    full = np.zeros((M, Kp), np.float32)
    full[:, :Kr] = cols
    Mp = (M + 31) // 32 * 32
    out = be.buf(np.full((Mp * Kp,), NAN_BITS, np.uint16))
    assert L.mgk_swin_im2col_pack(be.stream, be.p(be.buf(pix)), be.p(out), B, Cn, I, ps, Kp) == 0
    assert np.array_equal(out.numpy(), pk.pack_tiles(full))
    assert L.mgk_swin_im2col_pack(be.stream, be.p(be.buf(pix)), be.p(out), B, Cn, I, ps, Kr - 16 if Kr > 16 else 8) == MG_E_SHAPE


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("n,H", [(49, 2), (225, 8), (529, 32), (1, 1)])
def test_swin_transpose(be_name, n, H):
    be = get_backend(be_name)
    L = _lib(be)
    src = rs(n + H).standard_normal((n, H)).astype(np.float32)
    dst = be.buf(np.full((H, n), np.nan, np.float32))
    assert L.mgk_swin_transpose(be.stream, be.p(be.buf(src)), be.p(dst), n, H) == 0
    assert np.array_equal(dst.numpy(), src.T)
