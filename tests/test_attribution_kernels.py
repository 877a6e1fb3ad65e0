"""The cross-attention attribution kernel (csrc/k_attrib.hip) through its test entry mgk_xattn_map: the fp32 softmax of Q K^T over the
attended keys, summed over heads in registers and over layers in the scratch, gathered into [B][Sq][M_e1 + L + P].

Reference: float64 numpy on the same bf16 values, so the only difference is the kernel's fp32 arithmetic.  Bound: 1e-5 absolute on values
<= 1.  A probability's relative error is the absolute error of (s - max) plus a few ulp of exp2 and the normalisation: the random cases
use scores of a few units (fp32 accumulation of 64 bf16 products: about 1e-6), and the magnitude-80 case scripts Q and K on a grid of
sixteenths so that every score is exact in fp32 and what is left is exp2 of (s - m) * log2(e) - the rounding of that product matters only
where the probability itself is tiny."""
import ctypes as C

import numpy as np
import pytest

from tests import pkutil as pk
from tests.backends import get_backend

BACKENDS = [pytest.param("emu"), pytest.param("hip", marks=pytest.mark.gpu)]
TOL = 1e-5
SENT = np.float32(-77.25)


def _declare(lib):
    lib.mgk_xattn_map_scratch_bytes.restype = C.c_size_t
    lib.mgk_xattn_map_scratch_bytes.argtypes = [C.c_int] * 3
    lib.mgk_xattn_map.argtypes = [C.c_void_p] * 3 + [C.c_int] * 5 + [C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_size_t] + [C.c_int] * 4 + \
        [C.c_void_p] * 3


def _pack_heads(x, cap):
    """fp32 [B][H][S][64] -> HF_PK_ROWS bits [B][H][cap/32][4][512] (rows S .. cap zero)"""
    B, H, S, _ = x.shape
    return np.concatenate([pk.pack_tiles(x[b, h], rows_pad=cap).ravel() for b in range(B) for h in range(H)])


def _src_row(s, L, P, Lb):
    """output position s of [text L | patches P] -> workspace row of an image whose rows are [text Lb | patches P | text padding]"""
    return s if s < Lb else (Lb + P + (s - Lb) if s < L else Lb + (s - L))


def _run(be, qs, ks, mask, Sk_cap=None, Sq_cap=None, M_e1=0, M_pad=0, L=None, P=0, text_len=None, qmask=None, extra=5):
    """qs / ks: per layer fp32 [B][H][Sq][64] / [B][H][Sk][64] (bf16-exact), keys in workspace order [e1 slots M_pad | encoder rows];
    mask [B][Sk] u8.  One mgk_xattn_map per layer (store, then add; the last one scales and gathers) -> map [B][Sq][M_e1 + L + P]."""
    _declare(be.lib)
    B, H, Sq, _ = qs[0].shape
    Sk = ks[0].shape[2]
    L = Sk - M_pad - P if L is None else L
    assert M_pad + L + P == Sk
    Sk_cap = (Sk + 63) // 64 * 64 if Sk_cap is None else Sk_cap
    Sq_cap = (Sq + 31) // 32 * 32 if Sq_cap is None else Sq_cap
    km = np.zeros((B, Sk_cap), np.uint8)
    km[:, :Sk] = mask
    km[:, Sk:] = 1                                       # beyond Sk the mask must not be looked at
    nb = int(be.lib.mgk_xattn_map_scratch_bytes(B, Sq, Sk))
    assert nb == B * ((Sq + 31) // 32) * ((Sk + 31) // 32) * 4096
    scratch = be.buf(np.full(nb // 4, 0x7FC00000, np.uint32))          # (stale NaNs: the first layer stores)
    No = M_e1 + L + P
    out = be.buf(np.full(B * Sq * No + extra, SENT, np.float32))
    kmb = be.buf(km)
    tl = None if text_len is None else be.buf(np.asarray(text_len, np.int32))
    qm = None if qmask is None else be.buf(np.asarray(qmask, np.uint8))
    n = len(qs)
    for i, (q, k) in enumerate(zip(qs, ks)):
        rc = be.lib.mgk_xattn_map(be.stream, be.p(be.buf(_pack_heads(q, Sq_cap))), be.p(be.buf(_pack_heads(k, Sk_cap))), B, H, Sq, Sq_cap, Sk_cap,
                                  be.p(kmb), 1 if i else 0, 1.0 / (n * H) if i == n - 1 else 1.0, be.p(scratch), nb, M_e1, M_pad, L, P,
                                  be.p(tl), be.p(qm), be.p(out) if i == n - 1 else None)
        assert rc == 0
    res = out.numpy().copy()
    assert np.all(res[B * Sq * No:] == SENT), "written past the map"
    return res[:B * Sq * No].reshape(B, Sq, No)


def _ref(qs, ks, mask, M_e1=0, M_pad=0, L=None, P=0, text_len=None, qmask=None):
    B, H, Sq, _ = qs[0].shape
    Sk = ks[0].shape[2]
    L = Sk - M_pad - P if L is None else L
    acc = np.zeros((B, Sq, Sk))
    for q, k in zip(qs, ks):
        s = np.einsum("bhqd,bhkd->bhqk", q.astype(np.float64), k.astype(np.float64))
        s = np.where(mask[:, None, None, :] != 0, s, -np.inf)
        e = np.exp(s - s.max(-1, keepdims=True))
        acc += (e / e.sum(-1, keepdims=True)).sum(1)
    acc /= len(qs) * H
    cols = np.zeros((B, M_e1 + L + P), np.int64)
    for b in range(B):
        Lb = L if text_len is None else int(text_len[b])
        cols[b] = list(range(M_e1)) + [M_pad + _src_row(s, L, P, Lb) for s in range(L + P)]
    out = np.take_along_axis(acc, cols[:, None, :].repeat(Sq, 1), -1)
    if qmask is not None:
        out = out * (np.asarray(qmask)[..., None] != 0)
    return out, np.take_along_axis(np.asarray(mask), cols, -1)


def _qk(B, H, Sq, Sk, seed, scale=0.5):
    r = np.random.default_rng(seed)
    return (pk.bf16_round(r.standard_normal((B, H, Sq, 64)).astype(np.float32) * scale),
            pk.bf16_round(r.standard_normal((B, H, Sk, 64)).astype(np.float32)))


def _mask(B, Sk, seed, zero_first=True):
    m = (np.random.default_rng(seed).random((B, Sk)) < 0.7).astype(np.uint8)
    m[:, Sk - 1] = 1                                     # every image keeps an attended key
    if zero_first and Sk > 1:
        m[:, 0] = 0                                      # a masked key at index 0
    return m


def _check(got, ref, cmask, qmask=None):
    err = np.abs(got.astype(np.float64) - ref).max()
    live = np.ones(got.shape[:2], bool) if qmask is None else np.asarray(qmask) != 0
    sums = got.astype(np.float64).sum(-1)
    print(f"max abs error {err:.3e}; row sums off by {np.abs(sums[live] - 1).max():.3e}")
    assert err <= TOL
    assert np.abs(sums[live] - 1).max() <= TOL
    assert np.all(got[~live] == 0.0)
    assert np.all(got[np.broadcast_to((cmask == 0)[:, None, :], got.shape)] == 0.0)      # masked keys: exactly 0.0


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("Sq,Sk,H,B", [(1, 1, 1, 1), (31, 31, 3, 1), (32, 33, 1, 3), (33, 97, 3, 1), (65, 97, 16, 1), (65, 1, 3, 3),
                                       (1, 97, 1, 1), (33, 31, 16, 3), (32, 97, 3, 3), (31, 33, 1, 1)])
def test_shapes(be_name, Sq, Sk, H, B):
    """Sk 1 / 31 / 33 live in a 64-key capacity, 97 in 128; Sq 33 and 65 are two and three query tiles (workgroups) per image."""
    be = get_backend(be_name)
    q, k = _qk(B, H, Sq, Sk, 100 + Sq + Sk)
    mask = _mask(B, Sk, 7 + Sk)
    got = _run(be, [q], [k], mask)
    ref, cm = _ref([q], [k], mask)
    _check(got, ref, cm)


@pytest.mark.parametrize("be_name", BACKENDS)
def test_masked_tiles_and_query_mask(be_name):
    """Sk = 128 in four 32-key tiles: key 0 masked, tile 1 fully masked, tile 3 (trailing) fully masked; query rows 2 and 40 masked."""
    be = get_backend(be_name)
    B, H, Sq, Sk = 2, 3, 45, 128
    q, k = _qk(B, H, Sq, Sk, 31)
    mask = _mask(B, Sk, 32)
    mask[:, 32:64] = 0
    mask[:, 96:] = 0
    mask[:, 70] = 1
    qmask = np.ones((B, Sq), np.uint8)
    qmask[:, [2, 40]] = 0
    got = _run(be, [q], [k], mask, qmask=qmask)
    ref, cm = _ref([q], [k], mask, qmask=qmask)
    _check(got, ref, cm, qmask)


@pytest.mark.parametrize("be_name", BACKENDS)
def test_e1_block_and_padding_map(be_name):
    """Three e1 tokens in a 64-slot pad in front of L = 20 text and P = 13 visual rows; image b's workspace rows are [text Lb | patches |
    text padding] and the map's columns are [e1 3 | text 20 | patches 13]."""
    be = get_backend(be_name)
    B, H, Sq, M_e1, M_pad, L, P = 3, 3, 33, 3, 64, 20, 13
    text_len = [20, 12, 5]
    Sk = M_pad + L + P
    q, k = _qk(B, H, Sq, Sk, 41)
    mask = np.zeros((B, Sk), np.uint8)
    mask[:, :M_e1] = 1
    for b, Lb in enumerate(text_len):
        mask[b, M_pad:M_pad + Lb + P - 2] = 1            # text, then the kept patches; the last two visual slots dropped
    got = _run(be, [q], [k], mask, M_e1=M_e1, M_pad=M_pad, L=L, P=P, text_len=text_len)
    ref, cm = _ref([q], [k], mask, M_e1=M_e1, M_pad=M_pad, L=L, P=P, text_len=text_len)
    assert got.shape == (B, Sq, M_e1 + L + P)
    _check(got, ref, cm)
    assert np.all(cm[:, :M_e1] == 1) and np.all(got[:, :, :M_e1] > 0)
    for b, Lb in enumerate(text_len):
        assert np.all(got[b, :, M_e1 + Lb:M_e1 + L] == 0.0)          # the image's text padding, in the documented place
    same = _run(be, [q], [k], mask, M_e1=M_e1, M_pad=M_pad, L=L, P=P, text_len=None)
    assert np.array_equal(same[0], got[0])               # (text_len[0] = L: the identity map)


@pytest.mark.parametrize("be_name", BACKENDS)
def test_scores_of_magnitude_80(be_name):
    """Q and K on a grid of quarters (every product a sixteenth, every score exact in fp32).  Query t < 8 equals key 7 t + 3, so its own
    score is |k|^2 of about 90 against a field of about +-30; query 9 equals the LAST key (the largest score sits in the last key tile, after
    the running state of the earlier tiles has been built); query 10 equals a masked key (its peak must not count)."""
    be = get_backend(be_name)
    B, H, Sq, Sk = 1, 3, 33, 97
    r = np.random.default_rng(51)
    q = (r.integers(-8, 9, (B, H, Sq, 64)) / 4.0).astype(np.float32)
    k = (r.integers(-8, 9, (B, H, Sk, 64)) / 4.0).astype(np.float32)
    mask = _mask(B, Sk, 52)
    for t in range(8):
        q[:, :, t] = k[:, :, 7 * t + 3]
        mask[:, 7 * t + 3] = 1
    q[:, :, 9] = k[:, :, Sk - 1]
    q[:, :, 10] = k[:, :, 0]
    assert mask[0, 0] == 0
    s = np.einsum("bhqd,bhkd->bhqk", q.astype(np.float64), k.astype(np.float64))
    assert s[0, :, :8].max() > 80 and np.all(s == s.astype(np.float32))
    assert np.all(s[0, :, 9].argmax(-1) == Sk - 1)
    got = _run(be, [q], [k], mask)
    ref, cm = _ref([q], [k], mask)
    _check(got, ref, cm)
    assert np.all(got[0, 9, Sk - 1] > 0.99) and np.all(got[0, 10, 0] == 0.0)


@pytest.mark.parametrize("be_name", BACKENDS)
def test_store_then_add(be_name):
    """Two "layers": the second launch adds to what the first stored and applies 1 / (2 H); the result is the mean of the two single maps."""
    be = get_backend(be_name)
    B, H, Sq, Sk = 2, 3, 33, 70
    q0, k0 = _qk(B, H, Sq, Sk, 61)
    q1, k1 = _qk(B, H, Sq, Sk, 62)
    mask = _mask(B, Sk, 63)
    both = _run(be, [q0, q1], [k0, k1], mask)
    ref, cm = _ref([q0, q1], [k0, k1], mask)
    _check(both, ref, cm)
    a, b = _run(be, [q0], [k0], mask), _run(be, [q1], [k1], mask)
    assert np.abs(both.astype(np.float64) - (a.astype(np.float64) + b) / 2).max() <= 1e-6


@pytest.mark.parametrize("be_name", BACKENDS)
def test_an_image_does_not_depend_on_the_call(be_name):
    """Image 1 of a B = 3 call = the same image alone, bit for bit; so are its first 33 rows in a call of 33 rows."""
    be = get_backend(be_name)
    B, H, Sq, Sk = 3, 3, 65, 97
    q, k = _qk(B, H, Sq, Sk, 71)
    mask = _mask(B, Sk, 72)
    full = _run(be, [q], [k], mask)
    again = _run(be, [q], [k], mask)
    alone = _run(be, [q[1:2]], [k[1:2]], mask[1:2])
    short = _run(be, [q[1:2, :, :33]], [k[1:2]], mask[1:2])
    assert np.array_equal(full.view(np.uint32), again.view(np.uint32))
    assert np.array_equal(full[1].view(np.uint32), alone[0].view(np.uint32))
    assert np.array_equal(full[1, :33].view(np.uint32), short[0].view(np.uint32))


@pytest.mark.parametrize("be_name", BACKENDS)
def test_key_capacity_and_trailing_tiles_do_not_matter(be_name):
    """Sk = 64 in a capacity of 64 against the same keys in a capacity of 128, and against Sk = 128 with keys 64 .. 127 masked (two
    trailing tiles that contribute +0.0 to every row's sum): the same bits."""
    be = get_backend(be_name)
    B, H, Sq = 2, 3, 33
    q, k = _qk(B, H, Sq, 128, 81)
    mask = _mask(B, 128, 82)
    mask[:, 63] = 1
    mask[:, 64:] = 0
    a = _run(be, [q], [k[:, :, :64]], mask[:, :64], Sk_cap=64)
    b = _run(be, [q], [k[:, :, :64]], mask[:, :64], Sk_cap=128)
    c = _run(be, [q], [k], mask, Sk_cap=128)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(a.view(np.uint32), c[:, :, :64].view(np.uint32))
    assert np.all(c[:, :, 64:] == 0.0)


@pytest.mark.parametrize("be_name", BACKENDS)
def test_every_wave_partition(be_name):
    """Key-tile counts 9, 17, 25, 33 and 41 take 2 .. 6 tiles per wave; 1536 keys is the limit (48 tiles), 1537 is refused before any
    launch.  One head, one query tile: the partition is what is exercised."""
    be = get_backend(be_name)
    for Sk in (9 * 32 - 5, 17 * 32, 25 * 32 - 31, 33 * 32, 41 * 32 - 1, 1536):
        q, k = _qk(1, 1, 5, Sk, 90 + Sk % 7)
        mask = _mask(1, Sk, 91)
        got = _run(be, [q], [k], mask)
        ref, cm = _ref([q], [k], mask)
        _check(got, ref, cm)
    _declare(be.lib)
    z = be.zeros(64, np.uint8)
    assert be.lib.mgk_xattn_map(be.stream, be.p(z), be.p(z), 1, 1, 1, 32, 1600, None, 0, 1.0, be.p(z), 64, 0, 0, 1537, 0, None, None, None) == -5
    assert be.lib.mgk_xattn_map(be.stream, be.p(z), be.p(z), 1, 1, 1, 32, 64, None, 0, 1.0, be.p(z), 64, 0, 0, 33, 0, None, None, None) == -6
    assert be.lib.mgk_xattn_map(be.stream, be.p(z), be.p(z), 1, 1, 1, 32, 64, None, 0, 1.0, be.p(z), 64, 0, 0, 65, 0, None, None, None) == -1
