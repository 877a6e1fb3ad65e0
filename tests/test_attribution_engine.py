"""Attribution through the engine (include/mgrapher.h mg_decoder_attribute / mg_attribute_workspace_bytes; Engine.attribute /
Engine.attribute_candidates) on the tiny fixtures.

  references   A_fp32 = tests/attribution_script.AttrOracle in fp32, A_bf16 = the same with bf16 round trips at the engine's storage points.
               E_ref = max |A_bf16 - A_fp32| is what bf16 storage of the decoder's activations costs - computed here, on the CPU, from the
               references alone.  Asserted: |A_engine - A_fp32| <= 2 E_ref (the engine's rounding points - deferred norms, packed operands -
               are not the emulation's) and |A_engine - A_bf16| <= E_ref (the engine is closer to its emulation than the emulation to fp32)
  layers       [0, 0], [1, 1] and all: the all-layers map is the mean of the single-layer maps within 1e-6
  rows         decoder_attention_mask == 0: exactly 0.0; every other row sums to 1 within 1e-5; unattended keys exactly 0.0
  padding      per-image padding semantics: an image padded to a longer L in a batch = the image alone, bit for bit
  e1           the OCSR-branch tokens' columns come first
  candidates   [B, C, T] = C separate calls, bit for bit
  unchanged    forward_logits / score / generate give the same bits before and after attribute() and in a fresh engine that attributed
               first; mg_workspace_bytes and mg_score_workspace_bytes return the parent commit's numbers
  errors       MG_E_ARG / MG_E_SHAPE / MG_E_STATE / MG_E_WORKSPACE (and MG_E_INPUT for an image without an attended key)"""
import ctypes as C
import hashlib

import numpy as np
import pytest

from markushgrapher_amd import synth
from tests.attribution_script import AttrOracle
from tests.backends import make_engine
from tests.conftest import load_golden
from tests.test_oracle_golden import _inputs, _weights

BACKENDS = [pytest.param("emu"), pytest.param("hip", marks=pytest.mark.gpu)]
MG_E_SHAPE, MG_E_ARG, MG_E_STATE, MG_E_WORKSPACE, MG_E_INPUT = -1, -2, -3, -6, -8

# mg_workspace_bytes(model, B, L, 1, 0, T, 0) and mg_score_workspace_bytes(model, B, L, T, 0) of the tiny shape, recorded from the parent
# commit's emulator build: {(B, L, T): bytes}
PARENT_WS = {
    (1, 8, 0): 203520, (1, 8, 5): 347904, (1, 8, 64): 352000, (1, 8, 65): 463360,
    (1, 70, 0): 364032, (1, 70, 5): 541184, (1, 70, 64): 545280, (1, 70, 65): 656640,
    (3, 8, 0): 549120, (3, 8, 5): 973568, (3, 8, 64): 994048, (3, 8, 65): 1320192,
    (3, 70, 0): 1031168, (3, 70, 5): 1553920, (3, 70, 64): 1574400, (3, 70, 65): 1900544,
    (6, 8, 0): 1039360, (6, 8, 5): 1884160, (6, 8, 64): 1929216, (6, 8, 65): 2577152,
    (6, 70, 0): 2002944, (6, 70, 5): 3044352, (6, 70, 64): 3089408, (6, 70, 65): 3737344,
}
PARENT_SCORE_WS = {
    (1, 8, 5): 348672, (1, 8, 64): 353280, (1, 8, 65): 465152, (1, 70, 5): 541952, (1, 70, 64): 546560, (1, 70, 65): 658432,
    (3, 8, 5): 974336, (3, 8, 64): 997376, (3, 8, 65): 1324032, (3, 70, 5): 1554688, (3, 70, 64): 1577728, (3, 70, 65): 1904384,
    (6, 8, 5): 1884928, (6, 8, 64): 1935616, (6, 8, 65): 2584064, (6, 70, 5): 3045120, (6, 70, 64): 3095808, (6, 70, 65): 3744256,
}

_refs = {}


def _np(eng, h):
    return eng.mem.numpy(h)


def _case(be_name, fixture):
    g = load_golden(fixture)
    shape, sd = _weights(g)
    inp = _inputs(g, shape)
    eng = make_engine(be_name, shape, sd)
    args = (inp["input_ids"], inp["bbox"], inp["attention_mask"], inp["pixel_values"])
    labels = np.asarray(g["labels"]).astype(np.int64)
    dec = np.zeros_like(labels)
    dec[:, 1:] = labels[:, :-1]
    dec[:, 0] = shape.decoder_start_token_id
    dec[dec == -100] = shape.pad_token_id
    dam = (labels != -100).astype(np.uint8)
    return g, shape, sd, eng, args, labels, dec, dam


def _references(fixture, shape, sd, args, dec, dam):
    """(A_fp32, A_bf16) of the fixture, all layers: computed once and shared (read-only) by the backends' cases"""
    if fixture not in _refs:
        out = []
        for bf in (False, True):
            o = AttrOracle(shape, sd, emulate_bf16=bf)
            out.append(o.attribute(args[0], args[1], args[3], args[2], dec, dam.astype(np.int64)))
        for a in out:
            a.setflags(write=False)
        _refs[fixture] = tuple(out)
    return _refs[fixture]


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("fixture", ["g0_tiny.npz", "g3_trained_tiny.npz"])
def test_map_against_the_references(be_name, fixture):
    g, shape, sd, eng, args, labels, dec, dam = _case(be_name, fixture)
    a32, abf = _references(fixture, shape, sd, args, dec, dam)
    e_ref = np.abs(abf - a32).max()
    amap, enc_mask = eng.attribute(*args, dec, dam)
    amap, enc_mask = _np(eng, amap).copy(), _np(eng, enc_mask).copy()
    assert amap.shape == a32.shape and amap.dtype == np.float32
    e32, ebf = np.abs(amap - a32).max(), np.abs(amap - abf).max()
    print(f"{fixture} [{be_name}]: E_ref = max|A_bf16 - A_fp32| = {e_ref:.4e}; max|A_engine - A_fp32| = {e32:.4e}; "
          f"max|A_engine - A_bf16| = {ebf:.4e}; largest entry {a32.max():.3f}; attended keys {enc_mask.sum(-1).tolist()}")
    assert e32 <= 2 * e_ref
    assert ebf <= e_ref
    live = dam != 0
    assert np.all(amap[~live] == 0.0)
    assert np.abs(amap.astype(np.float64).sum(-1)[live] - 1).max() <= 1e-5
    assert np.all(amap[np.broadcast_to((enc_mask == 0)[:, None, :], amap.shape)] == 0.0)
    assert np.array_equal(enc_mask, np.asarray(g["enc_mask"]).astype(np.uint8))


@pytest.mark.parametrize("be_name", BACKENDS)
def test_layer_ranges(be_name):
    g, shape, sd, eng, args, labels, dec, dam = _case(be_name, "g3_trained_tiny.npz")
    assert shape.num_decoder_layers == 2
    full = _np(eng, eng.attribute(*args, dec, dam)[0]).copy()
    l0 = _np(eng, eng.attribute(*args, dec, dam, layers=(0, 0))[0]).copy()
    l1 = _np(eng, eng.attribute(*args, dec, dam, layers=1)[0]).copy()
    both = _np(eng, eng.attribute(*args, dec, dam, layers=(0, 1))[0]).copy()
    assert np.array_equal(full.view(np.uint32), both.view(np.uint32))
    assert np.abs(l0 - l1).max() > 1e-3                       # the layers differ
    assert np.abs(full.astype(np.float64) - (l0.astype(np.float64) + l1) / 2).max() <= 1e-6
    o = AttrOracle(shape, sd, emulate_bf16=True)
    r1 = o.attribute(args[0], args[1], args[3], args[2], dec, dam.astype(np.int64), layers=(1, 1))
    assert np.abs(l1 - r1).max() <= np.abs(l0 - r1).max() / 4      # the range selects the layer it names
    live = dam != 0
    for m in (l0, l1):
        assert np.abs(m.astype(np.float64).sum(-1)[live] - 1).max() <= 1e-5 and np.all(m[~live] == 0.0)


@pytest.mark.parametrize("be_name", BACKENDS)
def test_per_image_padding(be_name):
    """Per-image padding semantics: every image of a batch padded to L + 9 text slots against the image alone at its own text length."""
    g, shape, sd, eng, args, labels, dec, dam = _case(be_name, "g3_trained_tiny.npz")
    ids, bb, am, pix = (np.asarray(a) for a in args)
    B, L = ids.shape
    Lp = L + 9
    pid = np.zeros((B, Lp), ids.dtype); pid[:, :L] = ids
    pbb = np.zeros((B, Lp, 4), bb.dtype); pbb[:, :L] = bb
    pam = np.zeros((B, Lp), am.dtype); pam[:, :L] = am
    prev = eng.set_padding_semantics(True)
    try:
        batch = _np(eng, eng.attribute(pid, pbb, pam, pix, dec, dam)[0]).copy()
        for b in range(B):
            Lb = int(np.flatnonzero(am[b]).max()) + 1
            assert np.all(am[b, :Lb] != 0), "the fixture's text masks are prefixes"
            one = _np(eng, eng.attribute(ids[b:b + 1, :Lb], bb[b:b + 1, :Lb], am[b:b + 1, :Lb], pix[b:b + 1], dec[b:b + 1], dam[b:b + 1])[0])
            print(f"image {b}: Lb = {Lb}; max |batch - alone| = {np.abs(batch[b, :, :Lb] - one[0, :, :Lb]).max():.3e} (text), "
                  f"{np.abs(batch[b, :, Lp:] - one[0, :, Lb:]).max():.3e} (visual)")
            assert np.array_equal(batch[b, :, :Lb].view(np.uint32), one[0, :, :Lb].view(np.uint32)), b
            assert np.all(batch[b, :, Lb:Lp] == 0.0)
            assert np.array_equal(batch[b, :, Lp:].view(np.uint32), one[0, :, Lb:].view(np.uint32)), b
    finally:
        eng.set_padding_semantics(prev)


@pytest.mark.parametrize("be_name", BACKENDS)
def test_e1_columns_come_first(be_name):
    """The recipe e1 of tests/test_engine.py::test_e1_tokens_are_fused_into_the_cross_attention: five tokens in a 64-slot pad."""
    g, shape, sd, eng, args, labels, dec, dam = _case(be_name, "g3_trained_tiny.npz")
    B, M = args[0].shape[0], 5
    e1 = synth.round_bf16(synth.uniform_pm1("e1.tokens", (B, M, shape.d_model), 2) * np.float32(1.5))
    amap, enc_mask = eng.attribute(*args, dec, dam, e1=e1)
    amap, enc_mask = _np(eng, amap).copy(), _np(eng, enc_mask).copy()
    plain = _np(eng, eng.attribute(*args, dec, dam)[0])
    assert amap.shape[-1] == plain.shape[-1] + M and enc_mask.shape[-1] == plain.shape[-1]
    a32 = AttrOracle(shape, sd).attribute(args[0], args[1], args[3], args[2], dec, dam.astype(np.int64), e1=e1)
    abf = AttrOracle(shape, sd, emulate_bf16=True).attribute(args[0], args[1], args[3], args[2], dec, dam.astype(np.int64), e1=e1)
    e_ref = np.abs(abf - a32).max()
    print(f"e1: E_ref = {e_ref:.4e}; engine - fp32 {np.abs(amap - a32).max():.4e}; engine - bf16 {np.abs(amap - abf).max():.4e}; "
          f"e1 share {amap[..., :M].sum(-1)[dam != 0].mean():.3f}")
    assert np.abs(amap - a32).max() <= 2 * e_ref and np.abs(amap - abf).max() <= e_ref
    live = dam != 0
    assert np.all(amap[..., :M][live] > 0)                    # every e1 token is attended
    assert np.abs(amap.astype(np.float64).sum(-1)[live] - 1).max() <= 1e-5 and np.all(amap[~live] == 0.0)
    assert np.all(amap[..., M:][np.broadcast_to((enc_mask == 0)[:, None, :], plain.shape)] == 0.0)


@pytest.mark.parametrize("be_name", BACKENDS)
def test_candidates_equal_separate_calls(be_name):
    g, shape, sd, eng, args, labels, dec, dam = _case(be_name, "g3_trained_tiny.npz")
    cdec = np.stack([dec, np.roll(dec, 1, axis=0), dec[:, ::-1]], 1)
    cdec[:, :, 0] = shape.decoder_start_token_id
    cdam = np.stack([dam, np.ones_like(dam), np.roll(dam, 1, axis=0)], 1)
    out, msk = eng.attribute_candidates(*args, cdec, cdam, layers=(0, 1))
    out = _np(eng, out).copy()
    assert out.shape[:3] == cdec.shape
    for c in range(3):
        one, m1 = eng.attribute(*args, np.ascontiguousarray(cdec[:, c]), np.ascontiguousarray(cdam[:, c]))
        assert np.ascontiguousarray(out[:, c]).tobytes() == _np(eng, one).tobytes(), c
        assert np.array_equal(_np(eng, m1), _np(eng, msk))
    assert np.abs(out[:, 0] - out[:, 2]).max() > 1e-3


@pytest.mark.parametrize("be_name", BACKENDS)
def test_other_entry_points_are_unchanged(be_name):
    g, shape, sd, eng, args, labels, dec, dam = _case(be_name, "g3_trained_tiny.npz")
    T = 6                                                # (decode steps on the emulator are what this test's time goes to)

    def state(e):
        h = hashlib.sha256()
        h.update(_np(e, e.forward_logits(*args, dec)[0]).tobytes())
        for a in e.score(*args, dec, labels):
            h.update(_np(e, a).tobytes())
        h.update(_np(e, e.generate(*args, num_beams=1, max_length=T)[0]).tobytes())
        h.update(_np(e, e.generate(*args, num_beams=3, max_length=T)[0]).tobytes())
        return h.hexdigest()

    before = state(eng)
    first = _np(eng, eng.attribute(*args, dec, dam)[0]).copy()
    assert state(eng) == before                          # the same engine, after an attribute() call (its workspace grew in between)
    assert np.array_equal(_np(eng, eng.attribute(*args, dec, dam)[0]), first)      # and attribute() after the others
    _, _, _, eng2, _, _, _, _ = _case(be_name, "g3_trained_tiny.npz")
    assert np.array_equal(_np(eng2, eng2.attribute(*args, dec, dam)[0]), first)
    assert state(eng2) == before                         # a fresh engine that attributed first
    need = C.c_size_t()
    P = shape.num_patches
    for (B, L, T_), nbytes in PARENT_WS.items():
        assert eng.lib.mg_workspace_bytes(eng.model, B, L, 1, 0, T_, 0, C.byref(need)) == 0
        assert need.value == nbytes, (B, L, T_, need.value, nbytes)
        if T_ > 0:
            assert eng.lib.mg_score_workspace_bytes(eng.model, B, L, T_, 0, C.byref(need)) == 0
            assert need.value == PARENT_SCORE_WS[(B, L, T_)], (B, L, T_, need.value)
            assert eng.lib.mg_attribute_workspace_bytes(eng.model, B, L, T_, 0, C.byref(need)) == 0
            # the teacher-forced layout plus 4 bytes per (query, key), both rounded up to 32, plus the header
            tiles = B * ((T_ + 31) // 32) * ((L + P + 31) // 32)
            assert nbytes + tiles * 4096 + 256 <= need.value <= nbytes + tiles * 4096 + 256 + 512


@pytest.mark.parametrize("be_name", BACKENDS)
def test_errors(be_name):
    from markushgrapher_amd.engine import MgAttrOpts, MgError
    g, shape, sd, eng, args, labels, dec, dam = _case(be_name, "g3_trained_tiny.npz")
    B, T = dec.shape
    L = args[0].shape[1]
    mem, lib = eng.mem, eng.lib
    d_dec = mem.asarray(dec, np.int64)
    out = mem.empty((B, T, L + shape.num_patches), np.float32)

    def call(ws, nb, T_=T, opts=None):
        return lib.mg_decoder_attribute(eng.model, mem.stream(), mem.ptr(ws), nb, mem.ptr(d_dec), None, B, T_,
                                        C.byref(opts) if opts is not None else None, mem.ptr(out))

    # no prior encode on this workspace
    need = C.c_size_t()
    assert lib.mg_attribute_workspace_bytes(eng.model, B, L, T, 0, C.byref(need)) == 0
    ws = mem.empty((need.value,), np.uint8)
    assert call(ws, need.value) == MG_E_STATE
    # layer ranges
    for rng in ((-1, 0), (0, 2), (1, 0), (2, 2)):
        assert call(ws, need.value, opts=MgAttrOpts(*rng)) == MG_E_ARG, rng
        with pytest.raises(MgError, match=f"error {MG_E_ARG}:"):
            eng.attribute(*args, dec, dam, layers=rng)
    # T out of range (the engine of the tests decodes at most 64 positions)
    with pytest.raises(MgError, match=f"error {MG_E_SHAPE}:"):
        eng.attribute(*args, np.zeros((B, 65), np.int64))
    # a bad token id is reported as mg_decoder_score reports it, and the call after it is clean
    bad = dec.copy()
    bad[0, 1] = shape.vocab_size
    with pytest.raises(MgError, match=f"error {MG_E_INPUT}: .*token ids"):
        eng.attribute(*args, bad, dam)
    # an image without a single attended key: no text token attended, and one (unattended) token in every grid cell drops every patch
    eng.attribute(*args, dec, dam)
    n = shape.image_size // shape.patch_size
    c = (np.arange(n, dtype=np.float32) + 0.5) / n
    cx, cy = np.meshgrid(c, c)
    box = np.stack([cx.ravel() - 0.01, cy.ravel() - 0.01, cx.ravel() + 0.01, cy.ravel() + 0.01], -1).astype(np.float32)[None]
    ids0, am0 = np.full((1, n * n), 5, np.int64), np.zeros((1, n * n), np.int64)
    pv = np.asarray(args[3])[:1]
    assert not _np(eng, eng.encode(ids0, box, am0, pv)[1]).any()
    with pytest.raises(MgError, match=f"error {MG_E_INPUT}: .*attended"):
        eng.attribute(ids0, box, am0, pv, dec[:1], dam[:1])
    # a workspace sized for mg_decoder_forward only: too small for the map scratch
    eng.attribute(*args, dec, dam)                       # (leaves the encoder state of this batch in eng._ws)
    base = C.c_size_t()
    assert lib.mg_workspace_bytes(eng.model, B, L, 1, 0, T, 0, C.byref(base)) == 0
    assert call(eng._ws, base.value) == MG_E_WORKSPACE
    assert call(eng._ws, eng._ws_bytes) == 0
    assert call(eng._ws, eng._ws_bytes, T_=0) == MG_E_SHAPE
