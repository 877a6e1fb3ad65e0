"""The first-form attention kernel (attention_kernel<ATT_DEC_SELF> / <ATT_CROSS>, k_attn.hip) in the forms the engines launch it in: the
teacher-forced decoder forward (self with the T5 distance table, cross with the [e1 | encoder] key mask), the ChemicalOCR prefill (self over
the prompt, tab1_len = 1, left-aligned lengths) and the OCR vision tower (cross with a key mask; unmasked full frames take the bias-free
second form attention_enc_kernel<.., PLAIN>, whose dispatch boundary is covered here too).  All calls go through mgk_attention.

Reference: softmax attention per (b, h) in float64 numpy on the bf16-rounded operands (scale 0.5), masked and non-causal scores -1e30.
Only defined rows are compared: queries i < lens[b] (self), i < T (cross).

Tolerances (check_bounds), none of them taken from what the kernel gives:
  per element   |got - ref64| <= 3 * 2^-9 * max|V[b,h]|: bf16 rounding of the weights in the numerator, of the weights in the denominator
                and of the output, each at most 2^-9 relative, and a convex combination of value rows is bounded by max|v|
                (max over the Sk keys of the call; slots beyond Sk hold filler that must not be read into the result);
  mean          mean|got - ref64| <= 2 * mean|ref_model - ref64| over the same rows, ref_model = the kernel's rounding restated in numpy:
                P = bf16(exp(s - rowmax)), l = sum(P), o = bf16(P @ V / l).  The factor 2 is for what the model leaves out: the stage-wise
                running max, fast_exp and the fp32 accumulation order.

Every call (run_attention) is also the poison check: the context buffer is pre-filled with the bf16 NaN pattern 0x7FC0 and framed by one
row tile of guard on either side; every row < Sq_cap of every (b, h) must come back finite (later GEMMs read whole tiles) and both guards
must be untouched.

Measured: the numbers in brackets below are the ratio mean|got - ref64| / mean|ref_model - ref64| on the emulator | on an MI355X; the bound
is 2.  The two agree to the digits shown: what fast_exp and the accumulation order change stays below the bf16 rounding of the output.  Model
means were 1.5e-4 (512 keys) to 2.8e-4; the largest element error on the MI355X was 0.34 of the per-element bound
(test_self_ragged_cap[engine]).  No case needed a change in the kernel.

What each case reaches:
  test_self_ragged_cap[zero1]      T 300 of cap 320: three query blocks, the last one ragged (waves past the cap clamp their Q tile, stores
                                   guarded), per-block causal stage limit, lens 300 / 130 (ends inside a stage) / 1, tab1_len = 1: the OCR
                                   prefill's zero table (and the key-mask carve right behind a 1-entry table)      [0.986 | 0.986]
  test_self_ragged_cap[engine]     the same with the engine's table of T_cap distances                             [0.985 | 0.985]
  test_self_ragged_cap[clamp64]    tab1_len = 64 < T: distances clamp to the last entry                            [0.985 | 0.985]
  test_self_xcd_remap              B = 8, H = 3: the XCD-aware workgroup remap in ATT_DEC_SELF; every image bit-identical to the same
                                   operands in a B = 3 or B = 1 call (no remap)                                    [0.986 | 0.986]
  test_self_block_aligned_cap      T = cap = 256: two full query blocks, a length that ends exactly on a stage     [0.987 | 0.987]
  test_cross_masked_stages[256]    first stage wholly masked (the running max stays at the masked score, the weights exp(0) = 1 it
                                   accumulates must be wiped by the first real stage), mask ending inside a stage, a middle stage wholly
                                   masked, Sk 200 ending inside a stage                                            [0.974 | 0.974]
  test_cross_masked_stages[320]    the same with a whole stage of slots beyond Sk_pad; slots >= Sk hold 100.0      [0.977 | 0.977]
  test_cross_trailing_stage_masked last stage inside Sk wholly masked                                              [0.967 | 0.967]
  test_cross_e1_layout             the teacher-forced cross mask [1 x 144 | 0 x 48 | encoder mask] of pack_e1      [0.961 | 0.961]
  test_plain_boundary              S = 512 unmasked takes the second form; Sq = 511 or an all-ones mask fall back to the first form: all
                                   three against the reference, the two first-form calls bit-identical, first against second form within
                                   the per-element bound                              [second 0.961 | 0.961, first 0.962 | 0.962]
  test_cross_unmasked_cap_320      caps 320 (not a multiple of 256), unmasked: first form                          [0.966 | 0.966]
  test_entry_validation            MG_E_SHAPE for caps / lengths / modes the launcher does not take (host side, launches nothing)
"""
import functools

import numpy as np
import pytest

from tests import pkutil as pk
from tests.backends import get_backend
from tests.test_kernels import pack_heads_rows, pack_heads_t, rnd

BACKENDS = [pytest.param("emu"), pytest.param("hip", marks=pytest.mark.gpu)]
ATT_DEC_SELF, ATT_CROSS = 1, 2
MG_E_SHAPE = -1
NAN_BITS = 0x7FC0        # bf16 quiet NaN: what the context buffer holds before a launch
GUARD_BITS = 0xBEEF      # bf16 -0.4668: what the guard tiles around it hold, before and after
EPS_BF16 = 2.0 ** -9     # relative error of one round-to-nearest to bf16
NEG = -1e30


# ---------------------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------------------
def attend64(s, v):
    """(float64 softmax(s) @ v, the same with the kernel's three roundings) for scores s [nq][nk] and values v [nk][64]"""
    s, v = np.asarray(s, np.float64), np.asarray(v, np.float64)
    e = np.exp(s - s.max(-1, keepdims=True))
    ref = (e / e.sum(-1, keepdims=True)) @ v
    p = pk.bf16_round(e.astype(np.float32)).astype(np.float64)
    model = pk.bf16_round(((p @ v) / p.sum(-1, keepdims=True)).astype(np.float32)).astype(np.float64)
    return ref, model


def self_refs(q, k, v, T, lens, tab):
    """causal self-attention over keys j <= i, j < lens[b], bias tab[min(i - j, len(tab) - 1)][h]; rows >= lens[b] stay zero"""
    B, H = q.shape[:2]
    ref, model = np.zeros((B, H, T, 64)), np.zeros((B, H, T, 64))
    ii, jj = np.arange(T)[:, None], np.arange(T)[None, :]
    di = np.clip(ii - jj, 0, tab.shape[0] - 1)
    for b in range(B):
        n = int(lens[b])
        for h in range(H):
            s = q[b, h, :n].astype(np.float64) @ k[b, h, :n].astype(np.float64).T + tab[di[:n, :n], h].astype(np.float64)
            s = np.where(jj[:, :n] <= ii[:n], s, NEG)
            ref[b, h, :n], model[b, h, :n] = attend64(s, v[b, h, :n])
    return ref, model


def cross_refs(q, k, v, T, Sk, mask):
    B, H = q.shape[:2]
    ref, model = np.zeros((B, H, T, 64)), np.zeros((B, H, T, 64))
    for b in range(B):
        for h in range(H):
            s = q[b, h, :T].astype(np.float64) @ k[b, h, :Sk].astype(np.float64).T
            if mask is not None:
                s = np.where(mask[b, None, :Sk] != 0, s, NEG)
            ref[b, h], model[b, h] = attend64(s, v[b, h, :Sk])
    return ref, model


def t5_table(n, H, seed):
    """[n][H] by distance i - j, as the engine builds it for the causal decoder (bucket of -distance, 32 buckets, max distance 128)"""
    import torch
    from oracle.udop_oracle import relative_position_bucket as rpb
    return rnd((32, H), seed)[rpb(-torch.arange(0, n), False, 32, 128).numpy()].astype(np.float32)


def operands(shape, seed):
    return pk.bf16_round(rnd(shape, seed, 0.5))


# ---------------------------------------------------------------------------------------------------------------------------------
# one launch, with the poison check
# ---------------------------------------------------------------------------------------------------------------------------------
def run_attention(be, mode, q, k, v, Sq, Sk, kmask=None, tab=None):
    """mgk_attention on fp32 [B][H][cap][64] operands -> (fp32 [B][H][Sq_cap][64], stored bits uint16 [B][H][Sq_cap][64]).
    The context buffer starts as NaN between two guard tiles: asserts that every row comes back finite and the guards unchanged."""
    B, H, Sq_cap = q.shape[:3]
    Sk_cap = k.shape[2]
    HD = H * 64
    guard, rows = 32 * HD, B * Sq_cap
    buf = np.full((guard + rows * HD + guard,), GUARD_BITS, np.uint16)
    buf[guard:guard + rows * HD] = NAN_BITS
    ctx = be.buf(buf)
    Q, K, V = be.buf(pack_heads_rows(q)), be.buf(pack_heads_rows(k)), be.buf(pack_heads_t(v))
    import ctypes
    ctx_p = ctypes.c_void_p(ctx.ptr + guard * 2)
    rc = be.lib.mgk_attention(be.stream, mode, be.p(Q), be.p(K), be.p(V), ctx_p, B, H, Sq, Sk, Sq_cap, Sk_cap,
                              be.p(be.buf(kmask)) if kmask is not None else None,
                              be.p(be.buf(tab)) if tab is not None else None, 0 if tab is None else tab.shape[0],
                              None, None, None, None, None, None, None)
    assert rc == 0
    out = np.array(ctx.numpy(), copy=True)
    assert np.all(out[:guard] == GUARD_BITS), "written in front of the context buffer"
    assert np.all(out[guard + rows * HD:] == GUARD_BITS), "written behind the context buffer"
    bits = pk.unpack_tile_bits(out[guard:guard + rows * HD], HD).reshape(B, Sq_cap, H, 64).transpose(0, 2, 1, 3)
    got = pk.bf16_to_f32(bits)
    assert np.isfinite(got).all(), "rows left unwritten or not finite: %d" % int((~np.isfinite(got)).any(-1).sum())
    return got, np.ascontiguousarray(bits)


def check_bounds(name, got, ref, model, v, Sk, nrows):
    """nrows[b] defined query rows of image b.  Prints the figures, then asserts the per-element and the mean bound; returns the ratio."""
    B, H = ref.shape[:2]
    err_sum = mod_sum = 0.0
    count = 0
    worst = 0.0
    for b in range(B):
        n = int(nrows[b])
        for h in range(H):
            bound = 3 * EPS_BF16 * float(np.abs(v[b, h, :Sk]).max())
            e = np.abs(got[b, h, :n].astype(np.float64) - ref[b, h, :n])
            worst = max(worst, float(e.max()) / bound)
            err_sum += float(e.sum())
            mod_sum += float(np.abs(model[b, h, :n] - ref[b, h, :n]).sum())
            count += e.size
    mean_err, mean_mod = err_sum / count, mod_sum / count
    ratio = mean_err / mean_mod
    print("ATTN_PREFILL %s: mean err %.3e, model mean %.3e, ratio %.3f; max err / per-element bound %.3f"
          % (name, mean_err, mean_mod, ratio, worst))
    assert worst <= 1.0, "%s: an element is off by %.3f times the per-element bound" % (name, worst)
    assert mean_err <= 2 * mean_mod, "%s: mean error %.3e against the rounding model's %.3e (ratio %.3f > 2)" % (name, mean_err, mean_mod, ratio)
    return ratio


# ---------------------------------------------------------------------------------------------------------------------------------
# self-attention (ATT_DEC_SELF)
# ---------------------------------------------------------------------------------------------------------------------------------
LENS3 = [300, 130, 1]


def self_tab(form, T_cap, H):
    if form == "zero1":
        return np.zeros((1, H), np.float32)                       # the OCR prefill: no bias, a one-entry table of zeros
    if form == "engine":
        return t5_table(T_cap, H, 145)                            # the teacher-forced forward: one entry per distance of the cap
    return rnd((64, H), 146)                                      # clamp64: every entry distinct, so an off-by-one clamp shows


@functools.lru_cache(maxsize=None)
def self_case(B, H, T, T_cap, lens, form):
    """operands and references of one self-attention case, computed once for both backends (read-only from there on)"""
    q, k, v = [operands((B, H, T_cap, 64), 140 + i) for i in range(3)]
    mask = np.zeros((B, T_cap), np.uint8)
    for b in range(B):
        mask[b, :lens[b]] = 1
    tab = self_tab(form, T_cap, H)
    ref, model = self_refs(q, k, v, T, lens, tab)
    for a in (q, k, v, mask, tab, ref, model):
        a.setflags(write=False)
    return q, k, v, mask, tab, ref, model


def run_self(be, name, B, H, T, T_cap, lens, form):
    q, k, v, mask, tab, ref, model = self_case(B, H, T, T_cap, tuple(lens), form)
    got, bits = run_attention(be, ATT_DEC_SELF, q, k, v, T, T, kmask=mask, tab=tab)
    check_bounds(name, got, ref, model, v, T, lens)
    return bits


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("form", ["zero1", "engine", "clamp64"])
def test_self_ragged_cap(be_name, form):
    """B=3, H=2, T=300 of T_cap=320 (nqb = 3, the last block holds 64 rows: its waves 2, 3 clamp their Q tile and store nothing; causal
    stage limits 2, 4, 5 of 5), lens 300 / 130 / 1, with the table forms of the OCR prefill, the engine and a table shorter than T."""
    run_self(get_backend(be_name), "self_ragged[%s]" % form, 3, 2, 300, 320, LENS3, form)


@pytest.mark.parametrize("be_name", BACKENDS)
def test_self_xcd_remap(be_name):
    """B=8, H=3: B % 8 == 0 remaps the workgroup index (an image's heads and query blocks on one XCD) before it is decoded into
    (query block, head, image) - with H = 3 and nqb = 3 neither factor is a power of two.  Against the reference, and every image against
    the same operands in a call without the remap (B = 3, B = 3, B = 1, B = 1): the same bits on the defined rows."""
    be = get_backend(be_name)
    B, H, T, T_cap = 8, 3, 300, 320
    lens = [LENS3[b % 3] for b in range(B)]
    q, k, v, mask, tab, _, _ = self_case(B, H, T, T_cap, tuple(lens), "engine")
    bits8 = run_self(be, "self_xcd", B, H, T, T_cap, lens, "engine")
    for b0, n in ((0, 3), (3, 3), (6, 1), (7, 1)):
        sl = slice(b0, b0 + n)
        _, bits = run_attention(be, ATT_DEC_SELF, q[sl], k[sl], v[sl], T, T, kmask=mask[sl], tab=tab)
        for b in range(n):
            assert np.array_equal(bits[b, :, :lens[b0 + b]], bits8[b0 + b, :, :lens[b0 + b]]), "image %d differs from its B=%d call" % (b0 + b, n)


@pytest.mark.parametrize("be_name", BACKENDS)
def test_self_block_aligned_cap(be_name):
    """T = T_cap = 256: two full query blocks (no ragged block, no clamped wave), lens 256 / 64: the second image's keys end exactly on
    the first stage boundary, so every later stage of its rows is wholly masked."""
    run_self(get_backend(be_name), "self_aligned", 2, 3, 256, 256, [256, 64], "engine")


# ---------------------------------------------------------------------------------------------------------------------------------
# cross-attention (ATT_CROSS)
# ---------------------------------------------------------------------------------------------------------------------------------
FILL = 100.0             # what key / value slots >= Sk hold: large and finite; must not show in any result


@functools.lru_cache(maxsize=None)
def cross_case(name, B, H, T, T_cap, Sk, Sk_cap):
    q = operands((B, H, T_cap, 64), 150)
    k, v = [operands((B, H, Sk_cap, 64), 151 + i) for i in range(2)]
    k[:, :, Sk:] = FILL
    v[:, :, Sk:] = FILL
    mask = np.ones((B, Sk_cap), np.uint8)
    if name == "stages":
        mask[0, :70] = 0                     # first stage wholly masked, the mask ends inside the second
        mask[1, 64:128] = 0                  # a middle stage wholly masked
    elif name == "trailing":
        mask[:, 192:] = 0                    # the last stage inside Sk wholly masked
    elif name == "e1":                       # [144 e1 tokens | 48 padding slots up to M64 = 192 | encoder mask: S = 100 of S_cap = 128]
        mask[:, 144:192] = 0
        mask[1, 192 + 10:192 + 20] = 0       # (padding inside the second image's encoder sequence)
        mask[:, 192 + 100:] = 0
    elif name == "none":
        mask = None
    if mask is not None:
        mask[:, Sk:] = 0
    ref, model = cross_refs(q, k, v, T, Sk, mask)
    for a in (q, k, v, mask, ref, model):
        if a is not None:
            a.setflags(write=False)
    return q, k, v, mask, ref, model


def run_cross(be, label, name, B, H, T, T_cap, Sk, Sk_cap, Sq=None):
    q, k, v, mask, ref, model = cross_case(name, B, H, T, T_cap, Sk, Sk_cap)
    got, bits = run_attention(be, ATT_CROSS, q, k, v, T if Sq is None else Sq, Sk, kmask=mask)
    check_bounds(label, got, ref, model, v, Sk, [T] * B)
    return got, bits


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("Sk_cap", [256, 320])
def test_cross_masked_stages(be_name, Sk_cap):
    """B=2, H=2, T=150 of T_cap=192 (two query blocks, the second ragged), Sk=200 (ends inside the fourth stage).  Image 0: keys 0..69
    masked - the first stage accumulates 64 weights exp(0) = 1 over a running max that is still the masked score, and the first real
    stage must rescale them to nothing.  Image 1: keys 64..127 masked, a middle stage of zero weights.  Sk_cap = 320: one more whole stage of
    slots beyond Sk_pad that is never visited.  Slots >= Sk hold 100.0 in K and V (the reference never reads them)."""
    run_cross(get_backend(be_name), "cross_stages[%d]" % Sk_cap, "stages", 2, 2, 150, 192, 200, Sk_cap)


@pytest.mark.parametrize("be_name", BACKENDS)
def test_cross_trailing_stage_masked(be_name):
    """Sk = Sk_cap = 256, keys 192..255 masked: the last visited stage adds nothing."""
    run_cross(get_backend(be_name), "cross_trailing", "trailing", 2, 3, 150, 192, 256, 256)


@pytest.mark.parametrize("be_name", BACKENDS)
def test_cross_e1_layout(be_name):
    """The key layout of teacher-forced cross-attention with an attached vision branch: M64 = 192 slots of e1 tokens (144 real) in front of
    the encoder's S_cap = 128 positions (100 real): Sk = 292 of Sk_cap = 320, the third stage masked from its 17th key on."""
    run_cross(get_backend(be_name), "cross_e1", "e1", 2, 2, 150, 192, 192 + 100, 320)


@pytest.mark.parametrize("be_name", BACKENDS)
def test_plain_boundary(be_name):
    """B=1, H=2, S=512, no mask: the bias-free second form (attention()'s PLAIN dispatch: no mask, Sk == Sk_cap, Sq == Sq_cap, Sq_cap a
    multiple of 256).  Sq = 511 with the same caps, or an all-ones mask, break one condition each and take the first form."""
    be = get_backend(be_name)
    B, H, S = 1, 2, 512
    q, k, v, _, ref, model = cross_case("none", B, H, S, S, S, S)
    second, _ = run_attention(be, ATT_CROSS, q, k, v, S, S)
    check_bounds("plain_second_form", second, ref, model, v, S, [S] * B)
    short, short_bits = run_attention(be, ATT_CROSS, q, k, v, S - 1, S)
    check_bounds("plain_first_form[Sq=511]", short, ref, model, v, S, [S - 1] * B)
    ones, ones_bits = run_attention(be, ATT_CROSS, q, k, v, S, S, kmask=np.ones((B, S), np.uint8))
    check_bounds("plain_first_form[ones]", ones, ref, model, v, S, [S] * B)
    assert np.array_equal(short_bits[:, :, :S - 1], ones_bits[:, :, :S - 1])          # both are the first form: the same arithmetic
    for h in range(H):
        bound = 3 * EPS_BF16 * float(np.abs(v[0, h]).max())
        for first in (short, ones):
            assert np.abs(first[0, h, :S - 1] - second[0, h, :S - 1]).max() <= bound


@pytest.mark.parametrize("be_name", BACKENDS)
def test_cross_unmasked_cap_320(be_name):
    """Sq_cap = Sk_cap = 320, unmasked, full: everything the second form needs except a cap that is a multiple of 256 -> first form."""
    run_cross(get_backend(be_name), "cross_cap320", "none", 1, 2, 320, 320, 320, 320)


# ---------------------------------------------------------------------------------------------------------------------------------
# entry
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("be_name", BACKENDS)
def test_entry_validation(be_name):
    """mgk_attention refuses, before any launch: Sq_cap % 32, Sk_cap % 64, Sk > Sk_cap, Sq > Sq_cap, a mode outside 0..2."""
    be = get_backend(be_name)
    z = be.zeros((64,), np.uint16)

    def call(mode, Sq, Sk, Sq_cap, Sk_cap):
        return be.lib.mgk_attention(be.stream, mode, be.p(z), be.p(z), be.p(z), be.p(z), 1, 1, Sq, Sk, Sq_cap, Sk_cap,
                                    None, None, 0, None, None, None, None, None, None, None)
    for mode in (ATT_DEC_SELF, ATT_CROSS):
        assert call(mode, 40, 64, 48, 64) == MG_E_SHAPE          # Sq_cap % 32
        assert call(mode, 32, 64, 64, 96) == MG_E_SHAPE          # Sk_cap % 64
        assert call(mode, 32, 65, 64, 64) == MG_E_SHAPE          # Sk > Sk_cap
        assert call(mode, 65, 64, 64, 64) == MG_E_SHAPE          # Sq > Sq_cap
    assert call(3, 64, 64, 64, 64) == MG_E_SHAPE
    assert call(-1, 64, 64, 64, 64) == MG_E_SHAPE
    assert np.all(z.numpy() == 0)
