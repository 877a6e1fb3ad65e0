"""The stage in front of the first encoder GEMM and behind the last one, in every form mg_encode and the decode set-up run it: the input
assembly (embed_assemble, k_embed.hip), the bias bucket addresses (bias_index), the mask-derived lists and maps (attn_lists, row_tile_list,
pack_e1, the two enc_rows launches of the cross-attention stream, the output copies through enc_src_row) and the thin pack / gather kernels
(rmsnorm_pack[_rows], im2col_pack, pack_weight, embed_rows).  A bug here is a wrong index, not rounding noise, so nearly every assertion is
exact: integers, masks, float64 centres and bf16 / fp32 bit patterns against numpy restatements written in this file (float64 where the
operation rounds) and against the repository's own oracle (oracle/udop_oracle.py) where it covers the form.

Every case runs on the CPU SIMT emulator and, marked gpu, on the device (tests/backends.py)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from tests import pkutil as pk
from tests.backends import get_backend

BACKENDS = [pytest.param("emu"), pytest.param("hip", marks=pytest.mark.gpu)]
E_SHAPE, E_ARG = -1, -2
U24 = 2.0 ** -24                       # unit round-off of fp32
F32 = np.float32


def ci(x):
    return C.c_int(int(x))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class EmbedDesc(C.Structure):            # mgk_embed_desc (include/mgrapher.h)
    _fields_ = [(k, C.c_void_p) for k in ("input_ids", "bbox", "attention_mask", "patch_emb", "tok_emb", "x_emb", "y_emb")] + \
               [(k, C.c_int) for k in ("B", "L", "P", "d", "n_side", "M2", "V", "S_cap")] + \
               [("hidden", C.c_void_p), ("hidden_tiled", C.c_int), ("cx", C.c_void_p), ("cy", C.c_void_p), ("mask", C.c_void_p),
                ("xrow", C.c_void_p), ("xlen", C.c_void_p), ("x_row0", C.c_int), ("trim_padding", C.c_int), ("text_len", C.c_void_p),
                ("err", C.c_void_p), ("meta_ws", C.c_void_p)]


def vp(be, b):
    return None if b is None else be.p(b).value


# =========================================================================================================
# A. input assembly
# =========================================================================================================
D_A, V_A, M2_A = 64, 97, 1024


def assembly_inputs(n, B, L, bad_ids=False):
    """Token ids, boxes and embedding tables with the boxes built to hit the documented quirks of the combine (k_embed.hip header)."""
    rs = np.random.RandomState(1000 * n + 10 * L + B)
    P = n * n
    x0, y0 = rs.uniform(0.0, 0.9, (B, L)), rs.uniform(0.0, 0.9, (B, L))
    bbox = np.stack([x0, y0, np.minimum(x0 + rs.uniform(0.0, 0.2, (B, L)), 1.0), np.minimum(y0 + rs.uniform(0.0, 0.1, (B, L)), 1.0)], -1).astype(F32)
    c = (1.5 / n)
    for b in range(B):
        bbox[b, 0:3] = [c - 0.01 / n, c - 0.02 / n, c + 0.01 / n, c + 0.02 / n]      # several tokens under one patch
        bbox[b, 3] = 0.0                                                               # box mean exactly 0: drops patch 0, adds nothing
        bbox[b, 4] = 1.0                                                               # box mean exactly 1: drops the last patch, adds nothing
        bbox[b, 5] = [0.5, 1.5, 0.5, 1.5]                                              # mean exactly 1 with a centre elsewhere (and y > 1)
        bbox[b, 6] = [np.nextafter(F32(1), F32(2)), 1.0, 1.0, 1.0]                     # mean 1 + 2^-25 in float64 (but 1 in float32): a patch IS added
        for i, (kx, ky) in enumerate([(1, 2), (n - 1, 1), (n // 2, n // 2), (2, n - 1)]):
            bbox[b, 7 + i] = [F32(kx) / F32(n), F32(ky) / F32(n), F32(kx) / F32(n), F32(ky) / F32(n)]   # centres exactly on patch boundaries
        bbox[b, 11] = [0.0, 0.0, 1.0, 1.0]                                             # coordinates of exactly 0.0 and 1.0
        bbox[b, 12] = [-0.01, -0.02, 0.3, 0.4]                                         # slightly outside [0, 1]
        bbox[b, 13] = [0.99, 0.99, 1.05, 1.05]                                         # centre beyond the last patch
        bbox[b, 14] = [-0.3, -0.2, 0.1, 0.1]                                           # centre below patch 0
    for j in range(n):                                                                 # image 1: its text covers every patch of row 2 % n
        cx_, cy_ = (j + 0.5) / n, ((2 % n) + 0.5) / n
        bbox[1, 16 + j] = [cx_ - 0.1 / n, cy_ - 0.1 / n, cx_ + 0.1 / n, cy_ + 0.1 / n]
    assert 16 + n <= L
    ids = rs.randint(0, V_A, (B, L)).astype(np.int64)
    if bad_ids:
        ids[0, 15], ids[B - 1, 20], ids[B - 1, 21] = -1, V_A, V_A + 5
    return SimpleNamespace(
        n=n, B=B, L=L, P=P, d=D_A, ids=ids, bbox=bbox,
        patch=pk.bf16_round(rs.standard_normal((B, P, D_A)).astype(F32)) + F32(2.0 ** -12),     # (not bf16-exact: a real fp32 operand)
        tok=pk.bf16_round(rs.standard_normal((V_A, D_A)).astype(F32)),
        xe=pk.bf16_round(rs.standard_normal((M2_A, D_A)).astype(F32) * F32(0.5)),
        ye=pk.bf16_round(rs.standard_normal((M2_A, D_A)).astype(F32) * F32(0.5)))


def attention_mask(kind, B, L):
    if kind == "none":
        return None
    am = np.zeros((B, L), np.uint8)
    lens = {"trailing": [L, L - 7, 29], "interior": [L - 3, L, 31], "one_masked": [L - 5, 0, L]}[kind][:B]
    for b, n_ in enumerate(lens):
        am[b, :n_] = 1
    if kind == "interior":
        am[:, [2, 10, 17]] = 0
        am[0, L - 4] = 0                 # the token in front of the padding: the text length must come from the LAST attended token
    return am


def cell_index(v, M2):
    v = np.clip(np.asarray(v, np.float64), 0.0, 1.0)
    return np.clip((v * (M2 - 1)).astype(np.int64), 0, M2 - 1)


def ref_single(ids, bbox, am, b, n, M2, V):
    """ONE image with its own text of len(ids) tokens (stock combine_image_text_embeddings + get_visual_bbox + cell indices):
    per row of [text | surviving patches in raster order | zero visual slots] the token, the patch row of the batch, the four cell
    indices, the float64 box centre and the mask."""
    P = n * n
    x0, y0, x1, y1 = (bbox[:, i].astype(F32) for i in range(4))
    px = np.clip(np.floor((x0 + x1) / F32(2) * F32(n)), 0, n - 1).astype(np.int64)       # float32 arithmetic, floor, clip
    py = np.clip(np.floor((y0 + y1) / F32(2) * F32(n)), 0, n - 1).astype(np.int64)
    pt = px + py * n
    drop = np.zeros(P, bool)
    drop[pt] = True                                                                     # under EVERY text token, attended or not
    mean = (((x0.astype(np.float64) + y0.astype(np.float64)) + x1.astype(np.float64)) + y1.astype(np.float64)) / 4.0
    seg = (mean == 0.0) | (mean == 1.0)
    bad = (ids < 0) | (ids >= V)
    keep = np.flatnonzero(~drop)
    k = len(keep)
    vx0, vx1 = (keep % n).astype(F32) / F32(n), (keep % n + 1).astype(F32) / F32(n)       # float32 k / n, promoted to float64
    vy0, vy1 = (keep // n).astype(F32) / F32(n), (keep // n + 1).astype(F32) / F32(n)
    z = np.zeros(P - k, np.int64)
    cat = np.concatenate
    return SimpleNamespace(
        tok=cat([np.where(bad, 0, ids), -np.ones(P, np.int64)]), patch=cat([np.where(seg, -1, b * P + pt), b * P + keep, z - 1]),
        cells=np.stack([cat([cell_index(t, M2), cell_index(v, M2), z]) for t, v in ((x0, vx0), (y0, vy0), (x1, vx1), (y1, vy1))], -1),
        cx=cat([(x0.astype(np.float64) + x1.astype(np.float64)) / 2.0, (vx0.astype(np.float64) + vx1.astype(np.float64)) / 2.0, z * 0.0]),
        cy=cat([(y0.astype(np.float64) + y1.astype(np.float64)) / 2.0, (vy0.astype(np.float64) + vy1.astype(np.float64)) / 2.0, z * 0.0]),
        mask=cat([(am != 0) if am is not None else np.ones(len(ids), bool), np.ones(k, bool), np.full(P - k, am is None)]).astype(np.uint8),
        err=int(bad.sum()))


def ref_assemble(inp, am, S_cap, trim, x_row0):
    """The batch by the DEFINITION of the two padding semantics: every image assembled alone over its first Lb text tokens (Lb = L, or with
    trim_padding and a mask the index of its last attended text token + 1), the L - Lb padded slots moved behind the visual block
    (token 0, cell 0, not attended), rows >= L + P empty (cell index -1: zero hidden)."""
    B, L, P, d = inp.B, inp.L, inp.P, inp.d
    R = SimpleNamespace(tok=-np.ones((B, S_cap), np.int64), patch=-np.ones((B, S_cap), np.int64), cells=-np.ones((B, S_cap, 4), np.int64),
                        cx=np.zeros((B, S_cap)), cy=np.zeros((B, S_cap)), mask=np.zeros((B, S_cap), np.uint8), err=0,
                        text_len=np.zeros(B, np.int32))
    for b in range(B):
        Lb = L
        if trim and am is not None:
            nz = np.flatnonzero(am[b])
            Lb = int(nz[-1]) + 1 if len(nz) else 0
        one = ref_single(inp.ids[b, :Lb], inp.bbox[b, :Lb], None if am is None else am[b, :Lb], b, inp.n, M2_A, V_A)
        for k in ("tok", "patch", "cells", "cx", "cy", "mask"):
            getattr(R, k)[b, :Lb + P] = getattr(one, k)
        R.tok[b, Lb + P:L + P] = 0
        R.cells[b, Lb + P:L + P] = 0
        R.err += one.err
        R.text_len[b] = Lb
    rank = np.cumsum(R.mask, axis=1) - R.mask
    R.xrow = np.where(R.mask != 0, x_row0 + rank, -1).astype(np.int32)
    R.xlen = (x_row0 + R.mask.sum(1)).astype(np.int32)
    # hidden = (tok + patch) + (((x[l] + y[u]) + x[r]) + y[lo]): fp32 in the kernel's order, float64 and the bound of 5 roundings
    tok, patch, c = R.tok.reshape(-1), R.patch.reshape(-1), R.cells.reshape(-1, 4)
    patch_rows = inp.patch.reshape(-1, d)
    for dt in (np.float32, np.float64):
        t = np.where(tok[:, None] >= 0, inp.tok[np.maximum(tok, 0)].astype(dt), dt(0))
        p = np.where(patch[:, None] >= 0, patch_rows[np.maximum(patch, 0)].astype(dt), dt(0))
        tp = np.where(patch[:, None] >= 0, t + p, t)
        xe, ye, c0 = inp.xe.astype(dt), inp.ye.astype(dt), np.maximum(c, 0)
        s1 = xe[c0[:, 0]] + ye[c0[:, 1]]
        s2 = s1 + xe[c0[:, 2]]
        s3 = s2 + ye[c0[:, 3]]
        h = np.where(c[:, :1] >= 0, tp + s3, tp)
        if dt is np.float32:
            R.h32 = h.reshape(B, S_cap, d)
        else:
            R.h64 = h.reshape(B, S_cap, d)
            R.bound = (5 * U24 * np.max(np.abs([t, p, tp, s1, s2, s3, h]), axis=0)).reshape(B, S_cap, d)
    return R


class Assembler:
    """mgk_embed_assemble_ex on one set of inputs (uploaded once), outputs sentinel-filled before every call."""

    def __init__(self, be, inp, am, S_cap):
        self.be, self.inp, self.S_cap = be, inp, S_cap
        be.lib.mgk_embed_meta_bytes.restype = C.c_size_t
        self.meta = be.zeros((be.lib.mgk_embed_meta_bytes(inp.B, S_cap),), np.uint8)
        self.dev = [be.buf(inp.ids), be.buf(inp.bbox), None if am is None else be.buf(am), be.buf(inp.patch), be.buf(pk.bf16_bits(inp.tok)),
                    be.buf(pk.bf16_bits(inp.xe)), be.buf(pk.bf16_bits(inp.ye))]

    def __call__(self, trim=0, tiled=0, x_row0=0, want_text_len=True, S_cap=None, **over):
        be, inp = self.be, self.inp
        S_cap = self.S_cap if S_cap is None else S_cap
        B = inp.B
        o = SimpleNamespace(hidden=be.buf(np.full((B, self.S_cap, inp.d), 7.0, F32)), cx=be.buf(np.full((B, self.S_cap), 5.0)),
                            cy=be.buf(np.full((B, self.S_cap), 5.0)), mask=be.buf(np.full((B, self.S_cap), 9, np.uint8)),
                            xrow=be.buf(np.full((B, self.S_cap), 12345, np.int32)), xlen=be.buf(np.full((B,), 12345, np.int32)),
                            text_len=be.buf(np.full((B,), 12345, np.int32)), err=be.zeros((1,), np.int32))
        e = EmbedDesc(*[vp(be, x) for x in self.dev], B, inp.L, inp.P, inp.d, inp.n, M2_A, V_A, S_cap, vp(be, o.hidden), tiled, vp(be, o.cx),
                      vp(be, o.cy), vp(be, o.mask), vp(be, o.xrow), vp(be, o.xlen), x_row0, trim, vp(be, o.text_len) if want_text_len else None,
                      vp(be, o.err), vp(be, self.meta))
        for k, v in over.items():
            setattr(e, k, v)
        o.rc = be.lib.mgk_embed_assemble_ex(be.stream, C.byref(e))
        return o


def check_assembly(o, R, inp, S_cap, tiled, want_text_len):
    B, L, P, d = inp.B, inp.L, inp.P, inp.d
    assert o.rc == 0
    assert int(o.err.numpy()[0]) == R.err
    np.testing.assert_array_equal(o.mask.numpy(), R.mask)
    np.testing.assert_array_equal(o.cx.numpy(), R.cx)
    np.testing.assert_array_equal(o.cy.numpy(), R.cy)
    np.testing.assert_array_equal(o.xrow.numpy(), R.xrow)
    np.testing.assert_array_equal(o.xlen.numpy(), R.xlen)
    np.testing.assert_array_equal(o.text_len.numpy(), R.text_len if want_text_len else np.full(B, 12345))
    raw = o.hidden.numpy()
    hid = pk.untile_f32(raw.reshape(-1), d).reshape(B, S_cap, d) if tiled else raw
    assert np.all(np.isfinite(hid))
    for b in range(B):
        Lb = int(R.text_len[b])
        live = np.r_[0:Lb + P, L + P:S_cap]                     # the image's own rows and the empty tail: bit for bit
        np.testing.assert_array_equal(bits(hid[b, live]), bits(R.h32[b, live]))
        assert np.all(np.abs(hid[b, live].astype(np.float64) - R.h64[b, live]) <= R.bound[b, live])
        assert np.all(hid[b, L + P:] == 0) and np.all(R.cells[b, L + P:] == -1)
        moved = np.r_[Lb + P:L + P]                             # the moved text padding: not attended, never a cross-attention key, finite
        assert np.all(o.mask.numpy()[b, moved] == 0) and np.all(o.xrow.numpy()[b, moved] == -1)
    if tiled:                                                   # the tiled store: pkutil.tile_f32 of the row-major result, bit for bit
        ref = R.h32.copy()
        for b in range(B):
            m = np.r_[int(R.text_len[b]) + P:L + P]
            ref[b, m] = hid[b, m]
        np.testing.assert_array_equal(bits(raw.reshape(-1)), bits(pk.tile_f32(ref.reshape(B * S_cap, d))))


ASSEMBLY_SHAPES = [(4, 2, 48, 0), (4, 3, 200, 0), (17, 2, 48, 0), (17, 3, 200, 64), (32, 2, 48, 0), (32, 3, 200, 0)]      # n_side, B, L, extra padding


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("mask_kind", ["none", "trailing", "interior", "one_masked"])
@pytest.mark.parametrize("n,B,L,extra", ASSEMBLY_SHAPES)
def test_assembly_every_form(be_name, n, B, L, extra, mask_kind):
    """P = 16 / 289 / 1024 (1 / 2 with a ragged last thread / 4 patches per thread in the prefix sums; the last is the product's), text of 48
    and 200 tokens, S_cap = L + P rounded up to 64 (+ 64 of internal padding once), every combination of trim_padding, hidden_tiled,
    x_row0 in {0, 144} and text_len null / given, under no mask, trailing padding, interior zeros and one image fully masked.
    mask, cx, cy, xrow, xlen, text_len, err: exact.  Hidden rows: bit-equal to the fp32 restatement in the kernel's documented order
    (tok + patch) + (((x[l] + y[u]) + x[r]) + y[lo]), and within 5 roundings, 5 * 2^-24 * max |partial sum|, of the float64 value."""
    be = get_backend(be_name)
    inp, am = assembly_inputs(n, B, L), attention_mask(mask_kind, B, L)
    S_cap = (L + n * n + 63) // 64 * 64 + extra
    run = Assembler(be, inp, am, S_cap)
    refs = {trim: ref_assemble(inp, am, S_cap, trim, 0) for trim in (0, 1)}
    if am is not None:
        assert any(refs[1].text_len[b] < L for b in range(B))               # (the moved-padding branch runs)
    for trim in (0, 1):
        for tiled in (0, 1):
            for x_row0 in (0, 144):
                for want_tl in (False, True):
                    R = refs[trim]
                    R.xrow = np.where(R.mask != 0, x_row0 + np.cumsum(R.mask, axis=1) - R.mask, -1).astype(np.int32)
                    R.xlen = (x_row0 + R.mask.sum(1)).astype(np.int32)
                    check_assembly(run(trim, tiled, x_row0, want_tl), R, inp, S_cap, tiled, want_tl)


@pytest.mark.parametrize("mask_kind", ["none", "trailing"])
def test_assembly_reference_matches_the_oracle(mask_kind):
    """The numpy restatement above against the repository's oracle (combine + cell_embed, stock batched semantics = trim_padding 0): the same
    embeddings (same fp32 order), float64 boxes' centres and mask, at the three patch grids."""
    import torch
    from oracle.udop_oracle import Oracle
    for n, B, L in ((4, 2, 48), (17, 3, 200), (32, 2, 48)):
        inp, am = assembly_inputs(n, B, L), attention_mask(mask_kind, B, L)
        shape = SimpleNamespace(image_size=16 * n, patch_size=16, d_model=inp.d, max_2d_position_embeddings=M2_A, layer_norm_epsilon=1e-6)
        o = Oracle(shape, {"encoder.cell_2d_embedding.x_position_embeddings.weight": inp.xe,
                           "encoder.cell_2d_embedding.y_position_embeddings.weight": inp.ye})
        emb, bbox64, mask = o.combine(torch.from_numpy(inp.patch), torch.from_numpy(inp.tok[inp.ids]), torch.from_numpy(inp.bbox),
                                      None if am is None else torch.from_numpy(am.astype(np.int64)))
        cell, idx = o.cell_embed(bbox64)
        S = L + inp.P
        R = ref_assemble(inp, am, S, 0, 0)
        assert np.array_equal(R.h32, (emb + cell).numpy())
        np.testing.assert_array_equal(R.cx, bbox64[:, :, [0, 2]].mean(-1).numpy())
        np.testing.assert_array_equal(R.cy, bbox64[:, :, [1, 3]].mean(-1).numpy())
        np.testing.assert_array_equal(R.cells, idx.numpy())
        np.testing.assert_array_equal(R.mask, np.ones((B, S)) if am is None else mask.numpy())


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("trim", [0, 1])
def test_assembly_out_of_range_ids(be_name, trim):
    """Ids -1, V and V + 5: each counted in err and read as token 0 (the kernel's designed path; the engine turns err into MG_E_INPUT)."""
    be = get_backend(be_name)
    inp, am = assembly_inputs(17, 2, 48, bad_ids=True), attention_mask("trailing", 2, 48)
    S_cap = 384
    R = ref_assemble(inp, am, S_cap, trim, 0)
    assert R.err == 3
    o = Assembler(be, inp, am, S_cap)(trim, 0, 0, True)
    check_assembly(o, R, inp, S_cap, 0, True)
    hid = o.hidden.numpy()
    good = ref_assemble(SimpleNamespace(**{**vars(inp), "ids": np.where((inp.ids < 0) | (inp.ids >= V_A), 0, inp.ids)}), am, S_cap, trim, 0)
    np.testing.assert_array_equal(bits(hid[0, 15]), bits(good.h32[0, 15]))
    np.testing.assert_array_equal(bits(hid[1, 20:22]), bits(good.h32[1, 20:22]))


# =========================================================================================================
# B. bias index
# =========================================================================================================
KEY_OF_ENTRY = np.array([(e & 3) + 8 * ((e & 15) >> 2) + 4 * (e >> 4) for e in range(32)])      # accumulator key order of a 32-key tile
MASKED = 4 * 1024


def stock_bkhv():
    from oracle.udop_oracle import bucket_table
    return bucket_table(True, 32, 100, -100, 100).astype(np.int32)


def ref_buckets(c, bkhv, how="stock"):
    """[B][query][key] bucket of key - query: float64 difference -> float32 -> * float32(100) -> clamp to +-100 -> truncation -> table."""
    diff = c[:, None, :] - c[:, :, None]
    f = diff * 100.0 if how == "f64_product" else diff.astype(F32) * F32(100)       # (the near miss: the product and what follows in float64)
    f = np.clip(f, -100, 100)
    i = (np.floor(f) if how == "floor" else np.trunc(f)).astype(np.int64)
    return bkhv[i + 100].astype(np.int64)


def ref_bias_index(cx, cy, kmask, bkhv, Sk, how="stock"):
    B, S_cap = cx.shape
    v = 4 * (32 * ref_buckets(cy, bkhv, how) + ref_buckets(cx, bkhv, how))
    att = np.arange(S_cap)[None, :] < Sk
    if kmask is not None:
        att = att & (kmask != 0)
    v = np.where(att[:, None, :], v, MASKED)                                                # [B][q][key]
    keys = (np.arange(S_cap // 32)[:, None] * 32 + KEY_OF_ENTRY[None, :])                    # [kt][e]
    return np.ascontiguousarray(v[:, :, keys].transpose(0, 2, 1, 3)).astype(np.uint16)       # [B][kt][q][32]


def mixed_centres(B, S_cap, seed):
    """Patch centres (k + 0.5) / n built as the assembly builds them (float32 k / n, float64 mean), text centres from float32 coordinates,
    and the 101 values k / 100, whose differences * 100 sit on the integers where float32 / float64 and truncation / floor part."""
    rs = np.random.RandomState(seed)
    out = np.zeros((B, 2, S_cap))
    for b in range(B):
        for a in range(2):
            n = (32, 17)[(a + b) % 2]
            k = rs.randint(0, n, S_cap)
            patch = ((k.astype(F32) / F32(n)).astype(np.float64) + ((k + 1).astype(F32) / F32(n)).astype(np.float64)) / 2.0
            lo, w = rs.uniform(0, 0.9, S_cap).astype(F32), rs.uniform(0, 0.1, S_cap).astype(F32)
            text = (lo.astype(np.float64) + (lo + w).astype(np.float64)) / 2.0
            cent = rs.randint(0, 101, S_cap) / 100.0
            kind = rs.randint(0, 3, S_cap)
            c = np.where(kind == 0, patch, np.where(kind == 1, text, cent))
            if S_cap >= 101:
                c[:101] = rs.permutation(101) / 100.0            # every one of the 101 values, in no order
            out[b, a] = rs.permutation(c)
    return out[:, 0].copy(), out[:, 1].copy()


def all32_table():
    """A table in which every one of the 32 buckets occurs on both sides of distance 0 (the stock table never yields bucket 16: a
    positive distance is at least 1), and no two neighbouring distances share a bucket: every off-by-one in the distance shows."""
    d = np.arange(-100, 101)
    return ((d * 7 + 5) % 32).astype(np.int32)


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("table", ["stock", "all32"])
@pytest.mark.parametrize("S_cap,full", [(64, True), (64, False), (192, True), (192, False), (320, True), (320, False)])
def test_bias_index_exact(be_name, S_cap, full, table):
    """2 / 6 / 10 key tiles, B = 2, Sk = S_cap and Sk < S_cap, kmask null and with holes: the whole uint16 buffer [image][key tile][query][32]
    against the stock arithmetic restated in numpy.  The inputs are checked to tell the near misses apart (at S_cap = 320, on the
    reference alone): >= 100 pairs change bucket when the product is taken in float64, >= 1000 under floor instead of truncation, and every
    bucket of the table occurs in both directions - all 31 the stock table can yield (bucket 16 would need a positive distance below 1),
    all 32 with the second table, which also separates every pair of neighbouring distances."""
    be = get_backend(be_name)
    B = 2
    Sk = S_cap if full else S_cap - 23
    bkhv = stock_bkhv() if table == "stock" else all32_table()
    cx, cy = mixed_centres(B, S_cap, 7 + S_cap)
    rs = np.random.RandomState(S_cap)
    kmask = None if full else (rs.rand(B, S_cap) > 0.2).astype(np.uint8)
    if kmask is not None:
        kmask[:, Sk:] = 3                                        # bytes behind Sk are not attended whatever they hold
    ref = ref_bias_index(cx, cy, kmask, bkhv, Sk)
    if S_cap == 320:
        live = ref != MASKED
        assert np.count_nonzero((ref != ref_bias_index(cx, cy, kmask, bkhv, Sk, "f64_product")) & live) >= 100
        assert np.count_nonzero((ref != ref_bias_index(cx, cy, kmask, bkhv, Sk, "floor")) & live) >= 1000
        want = set(bkhv.tolist())
        assert len(want) == (31 if table == "stock" else 32)
        assert set((ref[live] // 4 % 32).tolist()) == want and set((ref[live] // 128).tolist()) == want
        assert np.count_nonzero(ref[live] // 128 != ref[live] // 4 % 32) > live.sum() // 2          # (vertical and horizontal differ: a swap shows)
    out = be.buf(np.full(ref.shape, 0xEEEE, np.uint16))
    assert be.lib.mgk_bias_index(be.stream, be.p(out), be.p(be.buf(cx)), be.p(be.buf(cy)), be.p(None if kmask is None else be.buf(kmask)), None,
                                 be.p(be.buf(bkhv)), B, Sk, S_cap) == 0
    np.testing.assert_array_equal(out.numpy(), ref)


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("n,L,trim", [(4, 48, 1), (17, 200, 0), (17, 200, 1)])
def test_bias_index_on_assembled_centres(be_name, n, L, trim):
    """cx / cy / mask as embed_assemble leaves them, fed to bias_index as mg_encode does: against the reference computed from the ORACLE's
    float64 boxes (per image alone over its own text when the padding is trimmed)."""
    import torch
    from oracle.udop_oracle import Oracle
    be = get_backend(be_name)
    B = 2
    inp, am = assembly_inputs(n, B, L), attention_mask("trailing", B, L)
    P, S = inp.P, L + inp.P
    S_cap = (S + 63) // 64 * 64
    o = Assembler(be, inp, am, S_cap)(trim, 1, 0, True)
    assert o.rc == 0
    shape = SimpleNamespace(image_size=16 * n, patch_size=16, d_model=inp.d, max_2d_position_embeddings=M2_A)
    orc = Oracle(shape, {})
    cx, cy, mask = np.zeros((B, S_cap)), np.zeros((B, S_cap)), np.zeros((B, S_cap), np.uint8)
    for b in range(B):
        Lb = int(am[b].sum()) if trim else L
        _, bbox64, m = orc.combine(torch.from_numpy(inp.patch[b:b + 1]), torch.zeros(1, Lb, inp.d), torch.from_numpy(inp.bbox[b:b + 1, :Lb]),
                                   torch.from_numpy(am[b:b + 1, :Lb].astype(np.int64)))
        cx[b, :Lb + P], cy[b, :Lb + P] = bbox64[0, :, [0, 2]].mean(-1).numpy(), bbox64[0, :, [1, 3]].mean(-1).numpy()
        mask[b, :Lb + P] = m[0].numpy()
    bkhv = stock_bkhv()
    ref = ref_bias_index(cx, cy, mask, bkhv, S)
    out = be.buf(np.full(ref.shape, 0xEEEE, np.uint16))
    assert be.lib.mgk_bias_index(be.stream, be.p(out), be.p(o.cx), be.p(o.cy), be.p(o.mask), None, be.p(be.buf(bkhv)), B, S, S_cap) == 0
    np.testing.assert_array_equal(out.numpy(), ref)


# =========================================================================================================
# C. lists and maps
# =========================================================================================================
def list_masks(kind, B, Sk, S_cap, seed):
    rs = np.random.RandomState(seed)
    m = np.ones((B, S_cap), np.uint8)
    if kind == "hole":                                           # a hole spanning whole stages (and parts of its neighbours)
        m[:, 40:min(Sk, 40 + S_cap * 3 // 5)] = 0
        m[1, :] = (rs.rand(S_cap) > 0.97)
        m[1, :64] = 0
    elif kind == "nothing":                                      # image 1: nothing attended
        m[1, :] = 0
        m[0, :] = (rs.rand(S_cap) > 0.5) * 2                     # (any non-zero byte attends)
    m[:, Sk:] = 0
    return m


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("kind", ["all", "hole", "nothing"])
@pytest.mark.parametrize("S_cap,cut", [(64, 0), (64, 30), (192, 0), (192, 70), (4480, 0), (4480, 200)])
def test_attn_lists_exact(be_name, S_cap, cut, kind):
    """1 / 3 (an odd count: the second query block has one stage) / 70 stages (more than the 64 threads), Sk = S_cap and below, with
    non-zero garbage in [Sk, S_cap) that must be ignored: kst = [count, ascending stage ids] ({1, 0} when nothing is attended, entries
    behind the count untouched) and qbv, exactly."""
    be = get_backend(be_name)
    B, Sk = 2, S_cap - cut
    m = list_masks(kind, B, Sk, S_cap, S_cap + cut)
    nstg, nqb = S_cap // 64, (S_cap + 127) // 128
    flag = np.zeros((B, 2 * nqb), bool)
    flag[:, :nstg] = m.reshape(B, nstg, 64).any(-1)
    kst_ref = np.full((B, 1 + nstg), -7, np.int32)
    for b in range(B):
        ids = np.flatnonzero(flag[b])
        if len(ids) == 0:
            ids = np.array([0])
        kst_ref[b, 0], kst_ref[b, 1:1 + len(ids)] = len(ids), ids
    if kind == "nothing":
        assert kst_ref[1, :2].tolist() == [1, 0] and not flag[1].any()
    m[:, Sk:] = 5                                                # garbage behind Sk
    kst, qbv = be.buf(np.full((B, 1 + nstg), -7, np.int32)), be.buf(np.full((B, nqb), 9, np.uint8))
    assert be.lib.mgk_attn_lists(be.stream, be.p(be.buf(m)), B, Sk, S_cap, be.p(kst), be.p(qbv)) == 0
    np.testing.assert_array_equal(kst.numpy(), kst_ref)
    np.testing.assert_array_equal(qbv.numpy(), flag.reshape(B, nqb, 2).any(-1).astype(np.uint8))


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("kind", ["random", "dead", "live", "last_byte"])
@pytest.mark.parametrize("n_tiles", [1, 40, 256, 257, 600])
def test_row_tile_list_exact(be_name, n_tiles, kind):
    """1 .. 600 tiles (up to 256: one per thread; 257: two per thread, 129 threads hold tiles; 600: three per thread, 200 threads): the list
    is the ascending ids of the tiles with a non-zero byte, the count its length ({0} / 1 when every tile is dead), entries behind the count
    keep the sentinel."""
    be = get_backend(be_name)
    rs = np.random.RandomState(n_tiles)
    m = np.zeros((n_tiles, 32), np.uint8)
    if kind == "random":
        m[rs.rand(n_tiles) > 0.6, rs.randint(0, 32)] = 1
        m[rs.rand(n_tiles) > 0.8] = 255
    elif kind == "live":
        m[:] = 1
    elif kind == "last_byte":
        m[n_tiles * 2 // 3, 31] = 128
    ids = np.flatnonzero(m.any(-1))
    ref = np.full(n_tiles + 1, -7, np.int32)
    if len(ids) == 0:
        ids = np.array([0])
    ref[:len(ids)] = ids
    lst, cnt = be.buf(np.full(n_tiles + 1, -7, np.int32)), be.buf(np.full(1, -7, np.int32))
    mb = be.buf(m)
    assert mb.ptr % 16 == 0
    assert be.lib.mgk_row_tile_list(be.stream, be.p(mb), n_tiles * 32, be.p(lst), be.p(cnt)) == 0
    assert int(cnt.numpy()[0]) == len(ids)
    np.testing.assert_array_equal(lst.numpy(), ref)


def halfway_values(shape, seed):
    """fp32 values with exact ties between two bf16 neighbours mixed in (round to nearest EVEN: both directions occur)."""
    x = np.random.RandomState(seed).standard_normal(shape).astype(F32)
    u = x.view(np.uint32).copy().reshape(-1)
    u[::5] = (u[::5] & 0xFFFF0000) | 0x8000                      # exactly halfway: rounds up when the kept mantissa is odd, down when even
    u[1::7] = (u[1::7] & 0xFFFF0000) | 0x7FFF                    # just below halfway
    return u.view(F32).reshape(shape)


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("with_xmask", [False, True])
@pytest.mark.parametrize("M,M_pad", [(5, 64), (144, 192)])
def test_pack_e1_and_the_cross_attention_stream(be_name, M, M_pad, with_xmask):
    """pack_e1 as mg_encode runs it (bf16 bits by round to nearest even, zero pad rows, row_map, xmask = [1 x M | 0 | encoder mask]), then
    the decode set-up's chain: xrow / xlen from the assembly at x_row0 = M and the two enc_rows launches into one sentinel-filled stream,
    which must be [e1 rows | attended encoder rows in order] bit for bit with the sentinel left in every row >= xlen[b]."""
    be = get_backend(be_name)
    B, d, n, L = 2, 64, 4, 48
    S_cap = 64
    inp, am = assembly_inputs(n, B, L), attention_mask("interior", B, L)
    o = Assembler(be, inp, am, S_cap)(1, 1, M, True)
    assert o.rc == 0
    mask = o.mask.numpy()
    natt = mask.astype(bool).sum(1)
    np.testing.assert_array_equal(o.xlen.numpy(), M + natt)
    e1 = halfway_values((B, M, d), M)
    e1_pk, rmap = be.buf(np.full((B * M_pad * d,), 0xABCD, np.uint16)), be.buf(np.full((B * M_pad,), -7, np.int32))
    xmask = be.buf(np.full((B, M_pad + S_cap), 9, np.uint8))
    assert be.lib.mgk_pack_e1(be.stream, be.p(be.buf(e1)), B, M, M_pad, d, be.p(e1_pk), be.p(rmap), be.p(o.mask), S_cap,
                              be.p(xmask) if with_xmask else None) == 0
    want = np.zeros((B, M_pad, d), np.uint16)
    want[:, :M] = pk.bf16_bits(e1)
    u = e1.view(np.uint32)
    tie = (u & 0xFFFF) == 0x8000
    assert np.any(want[:, :M][tie] == (u[tie] >> 16)) and np.any(want[:, :M][tie] == (u[tie] >> 16) + 1)      # ties went both ways
    np.testing.assert_array_equal(pk.unpack_tile_bits(e1_pk.numpy(), d), want.reshape(B * M_pad, d))
    np.testing.assert_array_equal(rmap.numpy().reshape(B, M_pad), np.tile(np.where(np.arange(M_pad) < M, np.arange(M_pad), -1), (B, 1)))
    if with_xmask:
        ref_x = np.zeros((B, M_pad + S_cap), np.uint8)
        ref_x[:, :M] = 1
        ref_x[:, M_pad:] = mask
        np.testing.assert_array_equal(xmask.numpy(), ref_x)
    else:
        assert np.all(xmask.numpy() == 9)
    Sx_cap = S_cap + M_pad
    enc = pk.bf16_bits(np.random.RandomState(3).standard_normal((B * S_cap, d)).astype(F32))
    dst = be.buf(np.full((B, Sx_cap, d), 0xABCD, np.uint16))
    assert be.lib.mgk_enc_rows(be.stream, be.p(e1_pk), be.p(rmap), be.p(dst), B, M_pad, Sx_cap, d) == 0
    assert be.lib.mgk_enc_rows(be.stream, be.p(be.buf(pk.pack_tile_bits(enc))), be.p(o.xrow), be.p(dst), B, S_cap, Sx_cap, d) == 0
    ref = np.full((B, Sx_cap, d), 0xABCD, np.uint16)
    for b in range(B):
        ref[b, :M] = want[b, :M]
        ref[b, M:M + natt[b]] = enc.reshape(B, S_cap, d)[b, mask[b] != 0]
        assert natt[b] < S_cap
    np.testing.assert_array_equal(dst.numpy(), ref)


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("lens", [None, (0, 48, 17)])
def test_enc_copy_out(be_name, lens):
    """The encoder's two output copies: rows and mask bytes in the documented [text L | patches P] order out of the workspace layout
    [text Lb | patches P | text padding L - Lb] (text_len null: Lb = L), Lb = 0 and Lb = L included: a numpy gather, exactly."""
    be = get_backend(be_name)
    B, L, P, d, S_cap = 3, 48, 16, 64, 128
    S = L + P
    rs = np.random.RandomState(11)
    enc, mask = rs.standard_normal((B, S_cap, d)).astype(F32), rs.randint(0, 256, (B, S_cap)).astype(np.uint8)
    src = np.zeros((B, S), np.int64)
    for b in range(B):
        Lb = L if lens is None else lens[b]
        src[b] = np.r_[0:Lb, Lb + P:L + P, Lb:Lb + P]            # text | its moved padding | patches
    tl = None if lens is None else be.buf(np.array(lens, np.int32))
    out, om = be.buf(np.full((B, S, d), 7.0, F32)), be.buf(np.full((B, S), 9, np.uint8))
    assert be.lib.mgk_enc_copy_out(be.stream, be.p(be.buf(enc)), be.p(be.buf(mask)), be.p(out), be.p(om), B, S, S_cap, d, L, be.p(tl)) == 0
    np.testing.assert_array_equal(bits(out.numpy()), bits(np.take_along_axis(enc, src[:, :, None], 1)))
    np.testing.assert_array_equal(om.numpy(), np.take_along_axis(mask, src, 1))
    # either output alone
    out2, om2 = be.buf(np.full((B, S, d), 7.0, F32)), be.buf(np.full((B, S), 9, np.uint8))
    assert be.lib.mgk_enc_copy_out(be.stream, be.p(be.buf(enc)), None, be.p(out2), None, B, S, S_cap, d, L, be.p(tl)) == 0
    assert be.lib.mgk_enc_copy_out(be.stream, None, be.p(be.buf(mask)), None, be.p(om2), B, S, S_cap, d, L, be.p(tl)) == 0
    assert np.array_equal(bits(out2.numpy()), bits(out.numpy())) and np.array_equal(om2.numpy(), om.numpy())


# =========================================================================================================
# D. the thin ones
# =========================================================================================================
def rms_bound_factor(d):
    """Relative error bound of the fp32 RMSNorm output in units of 2^-24, first order.  The sum of squares (all terms positive) goes
    through 1 product + 7 additions per 8-feature chunk, ceil(d / 512) chunk accumulations per lane and 6 wave-reduction levels:
    D = 14 + ceil(d / 512) roundings; / d and + eps add 2; the reciprocal square root halves that and adds its own error of at most one
    ulp = 2 units; the three products h * r, * gain, * scale add 3."""
    return (14 + -(-d // 512) + 2) / 2 + 2 + 3


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("scale", [1.0, 0.125])
@pytest.mark.parametrize("d", [64, 1024, 1536])
@pytest.mark.parametrize("M", [1, 37, 130])
def test_rmsnorm_pack_forms(be_name, M, d, scale):
    """d = 64 (56 of a wave's 64 lanes idle), 1024, 1536 (three chunks per lane); M = 1, 37, 130; scale 1 and not 1; out_f32 given and null;
    the dst_row form with skipped rows.  fp32 output within rms_bound_factor(d) * 2^-24 * |value| of float64; the packed output is the bf16
    rounding of the fp32 output bit for bit, the same bits with out_f32 null, rows >= M of the last tile and skipped rows untouched."""
    be = get_backend(be_name)
    rs = np.random.RandomState(M * 7 + d)
    h, g = (rs.standard_normal((M, d)) * 3).astype(F32), (1 + 0.2 * rs.standard_normal(d)).astype(F32)
    eps = 1e-6
    h64 = h.astype(np.float64)
    ref = g.astype(np.float64) * (h64 / np.sqrt((h64 ** 2).mean(-1, keepdims=True) + np.float64(F32(eps)))) * scale
    Mp = (M + 31) // 32 * 32
    hb, gb = be.buf(h), be.buf(g)
    xp, of = be.buf(np.full(Mp * d, 0xABCD, np.uint16)), be.buf(np.full((M, d), 7.0, F32))
    assert be.lib.mgk_rmsnorm_pack(be.stream, be.p(hb), be.p(gb), be.p(xp), be.p(of), M, d, C.c_float(eps), C.c_float(scale)) == 0
    got = of.numpy()
    assert np.all(np.abs(got.astype(np.float64) - ref) <= rms_bound_factor(d) * U24 * np.abs(ref))
    want = np.full((Mp, d), 0xABCD, np.uint16)
    want[:M] = pk.bf16_bits(got)
    np.testing.assert_array_equal(pk.unpack_tile_bits(xp.numpy(), d), want)
    xp2 = be.buf(np.full(Mp * d, 0xABCD, np.uint16))
    assert be.lib.mgk_rmsnorm_pack(be.stream, be.p(hb), be.p(gb), be.p(xp2), None, M, d, C.c_float(eps), C.c_float(scale)) == 0
    np.testing.assert_array_equal(xp2.numpy(), xp.numpy())
    # dst_row: a permutation into a larger buffer, every fifth row skipped
    Mq = Mp + 32
    dst_row = ((np.arange(M) * 7 + 3) % Mq).astype(np.int32) if M > 1 else np.array([Mq - 1], np.int32)
    assert len(set(dst_row.tolist())) == M
    dst_row[::5] = -1 - (np.arange(M)[::5] % 3)
    if M == 1:
        dst_row[0] = Mq - 1
    xp3 = be.buf(np.full(Mq * d, 0xABCD, np.uint16))
    assert be.lib.mgk_rmsnorm_pack_rows(be.stream, be.p(hb), be.p(gb), be.p(xp3), be.p(be.buf(dst_row)), M, d, C.c_float(eps), C.c_float(scale)) == 0
    want3 = np.full((Mq, d), 0xABCD, np.uint16)
    want3[dst_row[dst_row >= 0]] = want[:M][dst_row >= 0]
    np.testing.assert_array_equal(pk.unpack_tile_bits(xp3.numpy(), d), want3)


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("B,I", [(1, 48), (1, 512)])
def test_im2col_pack_shapes(be_name, B, I):
    """B * P = 9 rows (no multiple of 32: the padded rows of the only tile must be zero) and the product's 512-pixel page (1024 rows)."""
    be = get_backend(be_name)
    Cc, ps = 3, 16
    n = I // ps
    M, K = B * n * n, Cc * ps * ps
    pix = halfway_values((B, Cc, I, I), I)
    ref = pix.reshape(B, Cc, n, ps, n, ps).transpose(0, 2, 4, 1, 3, 5).reshape(M, K)
    Mp = (M + 31) // 32 * 32
    out = be.buf(np.full(Mp * K, 0xABCD, np.uint16))
    assert be.lib.mgk_im2col_pack(be.stream, be.p(be.buf(pix)), be.p(out), B, Cc, I, ps) == 0
    want = np.zeros((Mp, K), np.uint16)
    want[:M] = pk.bf16_bits(ref)
    np.testing.assert_array_equal(pk.unpack_tile_bits(out.numpy(), K), want)


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("K", [16, 4096])
def test_pack_weight_shapes(be_name, K):
    """fp32 and bf16 sources, N = 70 (no multiple of 32) into Npad = 128 > N + 32, one k-tile and 256: bf16 bits by round to nearest even,
    pad rows zero."""
    be = get_backend(be_name)
    N, Npad = 70, 128
    w = halfway_values((N, K), K)
    want = np.zeros((Npad, K), np.uint16)
    want[:N] = pk.bf16_bits(w)
    for src, is_bf16 in ((w, 0), (pk.bf16_bits(w), 1)):
        dst = be.buf(np.full(Npad * K, 0xABCD, np.uint16))
        assert be.lib.mgk_pack_weight(be.stream, be.p(be.buf(src)), is_bf16, N, K, be.p(dst), Npad) == 0
        np.testing.assert_array_equal(pk.unpack_tile_bits(dst.numpy(), K), want)


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("rows,d,x_ld,x_col0", [(37, 64, 96, 20), (130, 1024, 1024 + 64, 48), (5, 64, 64, 0)])
def test_embed_rows_and_its_packed_window(be_name, rows, d, x_ld, x_col0):
    """h = the table rows of the ids, exactly; ids -1 / V counted in err and read as row 0; the packed copy lands in columns [x_col0,
    x_col0 + d) of a wider buffer and touches nothing else; embed_norm_rows (the fused form of the decode step) leaves the same h bits."""
    be = get_backend(be_name)
    V = 97
    rs = np.random.RandomState(rows + d)
    tab = pk.bf16_bits(rs.standard_normal((V, d)).astype(F32))
    ids = rs.randint(0, V, rows).astype(np.int64)
    ids[1], ids[rows - 1] = -1, V
    safe = np.where((ids < 0) | (ids >= V), 0, ids)
    Rp = (rows + 31) // 32 * 32
    tb, ib = be.buf(tab), be.buf(ids)
    h, err, xw = be.buf(np.full((rows, d), 7.0, F32)), be.zeros((1,), np.int32), be.buf(np.full(Rp * x_ld, 0xABCD, np.uint16))
    assert be.lib.mgk_embed_rows(be.stream, be.p(ib), be.p(tb), be.p(h), rows, d, V, be.p(err), be.p(xw), x_ld, x_col0) == 0
    ref = pk.bf16_to_f32(tab[safe])
    np.testing.assert_array_equal(bits(h.numpy()), bits(ref))
    assert int(err.numpy()[0]) == 2
    np.testing.assert_array_equal(xw.numpy(), pk.window_bits(ref, x_ld, x_col0, 0xABCD, rows_pad=Rp))
    h1, err1 = be.buf(np.full((rows, d), 7.0, F32)), be.zeros((1,), np.int32)
    assert be.lib.mgk_embed_rows(be.stream, be.p(ib), be.p(tb), be.p(h1), rows, d, V, be.p(err1), None, 0, 0) == 0
    h2, err2, xn = be.buf(np.full((rows, d), 7.0, F32)), be.zeros((1,), np.int32), be.zeros((Rp * d,), np.uint16)
    gain = be.buf(np.ones(d, F32))
    assert be.lib.mgk_embed_norm_rows(be.stream, be.p(ib), be.p(tb), be.p(h2), be.p(gain), be.p(xn), None, 0, 0, rows, d, V, be.p(err2),
                                      C.c_float(1e-6)) == 0
    assert np.array_equal(bits(h1.numpy()), bits(ref)) and np.array_equal(bits(h2.numpy()), bits(ref))
    assert int(err1.numpy()[0]) == 2 and int(err2.numpy()[0]) == 2


# =========================================================================================================
# E. argument checks
# =========================================================================================================
@pytest.mark.parametrize("be_name", BACKENDS)
def test_argument_checks_come_before_any_device_work(be_name):
    """Every reject returns its documented code and leaves sentinel-filled outputs as they were."""
    be = get_backend(be_name)
    lib = be.lib
    sent = []

    def out(shape, dtype, fill):
        b = be.buf(np.full(shape, fill, dtype))
        sent.append((b, fill))
        return b

    # ---- embed_assemble_ex
    inp = assembly_inputs(4, 2, 48)
    run = Assembler(be, inp, None, 64)
    for kw, code in ((dict(S_cap=63), E_SHAPE), (dict(P=15), E_SHAPE), (dict(n_side=5), E_SHAPE), (dict(d=62), E_SHAPE), (dict(x_row0=-1), E_SHAPE),
                     (dict(hidden=None), E_ARG), (dict(meta_ws=None), E_ARG), (dict(input_ids=None), E_ARG), (dict(err=None), E_ARG),
                     (dict(xlen=None), E_ARG), (dict(B=0), E_SHAPE)):
        o = run(**kw)
        assert o.rc == code, kw
        assert np.all(o.hidden.numpy() == 7.0) and np.all(o.mask.numpy() == 9) and np.all(o.xrow.numpy() == 12345) and np.all(o.cx.numpy() == 5.0)
    inp17 = assembly_inputs(17, 2, 48)
    run17 = Assembler(be, inp17, None, 48 + 289)                 # S_cap = 337 = L + P: fine row-major, refused tiled
    assert run17(0, 0, 0, True).rc == 0
    o = run17(0, 1, 0, True)
    assert o.rc == E_SHAPE and np.all(o.hidden.numpy() == 7.0)
    assert lib.mgk_embed_assemble_ex(be.stream, None) == E_ARG
    # ---- bias_index / attn_lists / row_tile_list
    cx = be.buf(np.zeros((2, 128)))
    bk, km = be.buf(stock_bkhv()), be.buf(np.ones((2, 128), np.uint8))
    bo = out((2 * 4 * 128 * 32,), np.uint16, 0xEEEE)
    for args, code in (((2, 96, 96), E_SHAPE), ((2, 129, 128), E_SHAPE), ((0, 128, 128), E_SHAPE), ((2, -1, 128), E_SHAPE), ((2, 0, 0), E_SHAPE)):
        assert lib.mgk_bias_index(be.stream, be.p(bo), be.p(cx), be.p(cx), be.p(km), None, be.p(bk), *args) == code, args
    assert lib.mgk_bias_index(be.stream, None, be.p(cx), be.p(cx), None, None, be.p(bk), 2, 128, 128) == E_ARG
    assert lib.mgk_bias_index(be.stream, be.p(bo), None, be.p(cx), None, None, be.p(bk), 2, 128, 128) == E_ARG
    assert lib.mgk_bias_index(be.stream, be.p(bo), be.p(cx), be.p(cx), None, None, None, 2, 128, 128) == E_ARG
    kst, qbv = out((2, 3), np.int32, -7), out((2, 1), np.uint8, 9)
    for args, code in (((2, 96, 96), E_SHAPE), ((2, 129, 128), E_SHAPE), ((0, 128, 128), E_SHAPE)):
        assert lib.mgk_attn_lists(be.stream, be.p(km), *args, be.p(kst), be.p(qbv)) == code, args
    assert lib.mgk_attn_lists(be.stream, None, 2, 128, 128, be.p(kst), be.p(qbv)) == E_ARG
    assert lib.mgk_attn_lists(be.stream, be.p(km), 2, 128, 128, None, be.p(qbv)) == E_ARG
    assert lib.mgk_attn_lists(be.stream, be.p(km), 2, 128, 128, be.p(kst), None) == E_ARG
    lst, cnt = out((9,), np.int32, -7), out((1,), np.int32, -7)
    assert lib.mgk_row_tile_list(be.stream, be.p(km), 100, be.p(lst), be.p(cnt)) == E_SHAPE
    assert lib.mgk_row_tile_list(be.stream, be.p(km), 0, be.p(lst), be.p(cnt)) == E_SHAPE
    assert lib.mgk_row_tile_list(be.stream, C.c_void_p(km.ptr + 8), 64, be.p(lst), be.p(cnt)) == E_ARG       # the mask is read 16 bytes at a time
    assert lib.mgk_row_tile_list(be.stream, None, 64, be.p(lst), be.p(cnt)) == E_ARG
    assert lib.mgk_row_tile_list(be.stream, be.p(km), 64, None, be.p(cnt)) == E_ARG
    assert lib.mgk_row_tile_list(be.stream, be.p(km), 64, be.p(lst), None) == E_ARG
    # ---- pack_e1 / enc_copy_out
    e1 = be.buf(np.ones((2, 5, 64), F32))
    pko, rmo, xmo = out((2 * 64 * 64,), np.uint16, 0xABCD), out((2 * 64,), np.int32, -7), out((2, 64 + 128), np.uint8, 9)
    for (B, M, M_pad, d, S_cap), code in (((2, 5, 48, 64, 128), E_SHAPE), ((2, 5, 64, 60, 128), E_SHAPE), ((2, 5, 64, 72, 128), E_SHAPE),
                                          ((2, 5, 64, 64, 96), E_SHAPE), ((2, 65, 64, 64, 128), E_SHAPE), ((2, 0, 64, 64, 128), E_SHAPE),
                                          ((0, 5, 64, 64, 128), E_SHAPE)):
        assert lib.mgk_pack_e1(be.stream, be.p(e1), B, M, M_pad, d, be.p(pko), be.p(rmo), be.p(km), S_cap, be.p(xmo)) == code, (B, M, M_pad, d, S_cap)
    assert lib.mgk_pack_e1(be.stream, None, 2, 5, 64, 64, be.p(pko), be.p(rmo), be.p(km), 128, be.p(xmo)) == E_ARG
    assert lib.mgk_pack_e1(be.stream, be.p(e1), 2, 5, 64, 64, None, be.p(rmo), be.p(km), 128, be.p(xmo)) == E_ARG
    assert lib.mgk_pack_e1(be.stream, be.p(e1), 2, 5, 64, 64, be.p(pko), None, be.p(km), 128, be.p(xmo)) == E_ARG
    assert lib.mgk_pack_e1(be.stream, be.p(e1), 2, 5, 64, 64, be.p(pko), be.p(rmo), None, 128, be.p(xmo)) == E_ARG
    enc = be.buf(np.ones((2, 128, 64), F32))
    eo, mo = out((2, 100, 64), F32, 7.0), out((2, 100), np.uint8, 9)
    for (B, S, S_cap, d, L), code in (((2, 129, 128, 64, 48), E_SHAPE), ((2, 100, 128, 62, 48), E_SHAPE), ((2, 100, 128, 64, 101), E_SHAPE),
                                      ((2, 100, 128, 64, -1), E_SHAPE), ((0, 100, 128, 64, 48), E_SHAPE)):
        assert lib.mgk_enc_copy_out(be.stream, be.p(enc), be.p(km), be.p(eo), be.p(mo), B, S, S_cap, d, L, None) == code, (B, S, S_cap, d, L)
    assert lib.mgk_enc_copy_out(be.stream, be.p(enc), be.p(km), None, None, 2, 100, 128, 64, 48, None) == E_ARG
    assert lib.mgk_enc_copy_out(be.stream, None, be.p(km), be.p(eo), be.p(mo), 2, 100, 128, 64, 48, None) == E_ARG
    assert lib.mgk_enc_copy_out(be.stream, be.p(enc), None, be.p(eo), be.p(mo), 2, 100, 128, 64, 48, None) == E_ARG
    # ---- embed_rows / rmsnorm_pack_rows
    ids, tab, errb = be.buf(np.zeros(4, np.int64)), be.buf(np.zeros((8, 64), np.uint16)), out((1,), np.int32, 0)
    ho, xo = out((4, 64), F32, 7.0), out((32 * 96,), np.uint16, 0xABCD)
    for (rows, d, V, x_ld, x_col0), code in (((0, 64, 8, 96, 0), E_SHAPE), ((4, 62, 8, 96, 0), E_SHAPE), ((4, 64, 0, 96, 0), E_SHAPE),
                                             ((4, 64, 8, 88, 0), E_SHAPE), ((4, 64, 8, 96, 34), E_SHAPE), ((4, 64, 8, 96, 36), E_SHAPE),
                                             ((4, 64, 8, 96, -4), E_SHAPE)):
        assert lib.mgk_embed_rows(be.stream, be.p(ids), be.p(tab), be.p(ho), rows, d, V, be.p(errb), be.p(xo), x_ld, x_col0) == code, (rows, d, x_ld, x_col0)
    assert lib.mgk_embed_rows(be.stream, None, be.p(tab), be.p(ho), 4, 64, 8, be.p(errb), None, 0, 0) == E_ARG
    assert lib.mgk_embed_rows(be.stream, be.p(ids), be.p(tab), None, 4, 64, 8, be.p(errb), None, 0, 0) == E_ARG
    assert lib.mgk_embed_rows(be.stream, be.p(ids), be.p(tab), be.p(ho), 4, 64, 8, None, None, 0, 0) == E_ARG
    hh, gg = be.buf(np.ones((4, 64), F32)), be.buf(np.ones(64, F32))
    for (M, d), code in (((0, 64), E_SHAPE), ((4, 72), E_SHAPE), ((4, 8), E_SHAPE)):
        assert lib.mgk_rmsnorm_pack_rows(be.stream, be.p(hh), be.p(gg), be.p(xo), None, M, d, C.c_float(1e-6), C.c_float(1.0)) == code, (M, d)
    assert lib.mgk_rmsnorm_pack_rows(be.stream, None, be.p(gg), be.p(xo), None, 4, 64, C.c_float(1e-6), C.c_float(1.0)) == E_ARG
    assert lib.mgk_rmsnorm_pack_rows(be.stream, be.p(hh), None, be.p(xo), None, 4, 64, C.c_float(1e-6), C.c_float(1.0)) == E_ARG
    assert lib.mgk_rmsnorm_pack_rows(be.stream, be.p(hh), be.p(gg), None, None, 4, 64, C.c_float(1e-6), C.c_float(1.0)) == E_ARG
    for b, fill in sent:
        assert np.all(b.numpy() == fill)
