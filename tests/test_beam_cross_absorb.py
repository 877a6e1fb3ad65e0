"""Weight-absorbed cross-attention for beam search (include/mgrapher.h mg_set_beam_cross_absorb; k_xattn.hip xattn_beams_kernel).

The beam form streams the states of an image once for several of its beams.  Its contract is the per-row stream kernel's bits: for every
row it must write what xattn_stream_kernel writes at the same key splits / ring, so the kernel tests below compare mgk_xattn_beams with
mgk_xattn bit for bit.  The engine tests hold the form to the fixtures' tolerances and to the row independence the queue relies on.
`emu` = the same sources on the CPU SIMT emulator (shapes shrunk), `hip` = the MI355X (marked gpu)."""
import ctypes as C

import numpy as np
import pytest

from tests import pkutil as pk
from tests.backends import get_backend, make_engine
from tests.conftest import load_golden
from tests.test_oracle_golden import _weights, _inputs

BACKENDS = [pytest.param("emu"), pytest.param("hip", marks=pytest.mark.gpu)]


def rnd(shape, seed, scale=1.0):
    return (np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32)


def softmax_ref(x):
    x = x - x.max(axis=-1, keepdims=True)
    e = np.exp(x)
    return e / e.sum(axis=-1, keepdims=True)


def _bps(d, nstg):
    """Beams per workgroup the kernel supports for a width and ring (k_xattn.hip xattn_beams_bp)."""
    return (2, 3) if nstg == 3 and d <= 768 else (2,)


class _Case:
    """One problem: `len(lens)` images of `group` beams, image i's rows read owner kv_img[i]."""

    def __init__(self, be, d, H, group, cap, lens, seed=0, kv_img=None):
        self.be, self.d, self.H, self.group, self.cap = be, d, H, group, cap
        self.lens = np.asarray(lens, np.int32)
        n = len(lens)
        self.kv_img = np.asarray(kv_img if kv_img is not None else [(i + 1) % n for i in range(n)], np.int32)
        self.rows = n * group
        self.kv_row = np.repeat(self.kv_img, group).astype(np.int32)
        inner = H * 64
        self.q = pk.bf16_round(rnd((self.rows, H, 64), 100 + seed, 0.5))
        self.wkv = pk.bf16_round(rnd((2 * inner, d), 101 + seed, 1.0 / np.sqrt(d)))
        self.enc = pk.bf16_round(rnd((n, cap, d), 102 + seed, 1.0))
        self.Q, self.W = be.buf(pk.bf16_bits(self.q)), be.buf(self.wkv)
        self.L, self.KVI, self.KVR = be.buf(self.lens), be.buf(self.kv_img), be.buf(self.kv_row)
        self.E = be.buf(pk.bf16_bits(self.enc))

    def run(self, nsplit, nstg, bp=None, live=None, enc=None, part_fill=0, kv_img=True, nt=1):
        """bp None: the per-row kernel (mgk_xattn, kv_owner per row); else mgk_xattn_beams.  Returns (ctx, part, ml) as arrays."""
        be, rows, H, d = self.be, self.rows, self.H, self.d
        inner = H * 64
        ctx = be.zeros((((rows + 31) // 32 * 32) * inner,), np.uint16)
        wk, wv = be.zeros((H * d * 64,), np.uint16), be.zeros((H * d * 64,), np.uint16)
        qx = be.zeros((rows * H * d,), np.uint16)
        part = be.buf(np.full((rows * nsplit * H * d,), part_fill, np.uint16))
        ml = be.buf(np.full((rows * nsplit * H * 2,), np.float32(part_fill), np.float32))
        E = self.E if enc is None else be.buf(pk.bf16_bits(enc))
        if bp is None:
            rc = be.lib.mgk_xattn(be.stream, be.p(self.Q), be.p(self.W), be.p(E), be.p(self.L), be.p(self.KVR), rows, H, d, self.cap,
                                  nsplit, nstg, be.p(wk), be.p(wv), be.p(qx), be.p(part), be.p(ml), be.p(ctx))
        else:
            rc = be.lib.mgk_xattn_beams(be.stream, be.p(self.Q), be.p(self.W), be.p(E), be.p(self.L), be.p(self.KVI) if kv_img else None,
                                        be.p(be.buf(live)) if live is not None else None, rows, H, d, self.cap, self.group, nsplit, nstg, bp, nt,
                                        be.p(wk), be.p(wv), be.p(qx), be.p(part), be.p(ml), be.p(ctx))
        assert rc == 0, rc
        return (np.array(ctx.numpy(), copy=True), np.array(part.numpy(), copy=True), np.array(ml.numpy(), copy=True).view(np.uint32))

    def ctx_f32(self, ctx):
        return pk.unpack_tiles(ctx, self.rows, self.H * 64).reshape(self.rows, self.H, 64)


def _shapes(be_name, d):
    if be_name == "emu" and d >= 768:
        return 48, [48, 19]
    if be_name == "emu":
        return 64, [64, 1, 37]
    return 160, [160, 37, 1, 16, 97]


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("group", [2, 3, 5])
@pytest.mark.parametrize("d,H", [(64, 2), (256, 4), (768, 12), (1024, 16)])
def test_beam_stream_bits_equal_per_row_stream(be_name, d, H, group):
    """mgk_xattn_beams against mgk_xattn with kv_owner[r] = owner(r // group), bit for bit (context, split partials, (m, l)), for every
    supported beams-per-workgroup, key splits 1..3 and both rings.  Lengths cover one key, a partial stage, whole stages, the capacity."""
    be = get_backend(be_name)
    cap, lens = _shapes(be_name, d)
    case = _Case(be, d, H, group, cap, lens, seed=group)
    splits = (1, 3) if be_name == "emu" and d >= 768 else (1, 2, 3)
    for nstg in (3, 4):
        for nsplit in splits:
            ref = case.run(nsplit, nstg)
            for bp in _bps(d, nstg) + (0,):
                got = case.run(nsplit, nstg, bp=bp)
                for a, b, what in zip(got, ref, ("ctx", "part", "ml")):
                    assert np.array_equal(a, b), (what, nstg, nsplit, bp)
    # the batch form's owner rule (kv_owner null: row r reads image r // group)
    ident = _Case(be, d, H, group, cap, lens, seed=group, kv_img=np.arange(len(lens)))
    assert np.array_equal(ident.run(1, 4, bp=0, kv_img=False)[0], ident.run(1, 4)[0])


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("d,H", [(64, 2), (256, 4), (1024, 16)])
def test_beam_stream_against_stock_formulation(be_name, d, H):
    """The beam form against fp32 numpy of stock's K = enc Wk^T, V = enc Wv^T, softmax(q K^T) V (modeling_udop.py:524-575), within the
    bound of test_kernels.py::test_absorbed_cross_attention; the result must not match another head's or row's reference."""
    be = get_backend(be_name)
    cap, lens = _shapes(be_name, d)
    case = _Case(be, d, H, 5, cap, lens, seed=7)
    inner = H * 64
    got = case.ctx_f32(case.run(2, 4, bp=0)[0])
    ref, kvf = np.zeros_like(got), np.zeros_like(got)
    for r in range(case.rows):
        o = case.kv_row[r]
        n = case.lens[o]
        for h in range(H):
            K = case.enc[o, :n] @ case.wkv[h * 64:(h + 1) * 64].T
            V = case.enc[o, :n] @ case.wkv[inner + h * 64:inner + (h + 1) * 64].T
            ref[r, h] = softmax_ref((K @ case.q[r, h])[None])[0] @ V
            Kb, Vb = pk.bf16_round(K), pk.bf16_round(V)
            kvf[r, h] = pk.bf16_round(pk.bf16_round(softmax_ref((Kb @ case.q[r, h])[None])[0]) @ Vb)
    e_abs, e_kv = np.abs(got - ref), np.abs(kvf - ref)
    assert e_abs.max() <= 2.0 * e_kv.max() + 2e-3 and e_abs.mean() <= 2.0 * e_kv.mean() + 2e-4, (e_abs.max(), e_kv.max())
    # (25 rows here against that test's 7: the element-wise bound gets the tail of more samples - 3e-2 instead of 2e-2)
    np.testing.assert_allclose(got, ref, rtol=1 / 32, atol=3e-2)
    assert np.abs(got - np.roll(ref, 1, axis=1)).max() > 0.05 and np.abs(got - np.roll(ref, 1, axis=0)).max() > 0.05


@pytest.mark.parametrize("be_name", BACKENDS)
def test_beam_stream_cache_policy_keeps_the_bits(be_name):
    """The copies' cache policy (non-temporal or default) is a speed choice only: same bits."""
    be = get_backend(be_name)
    case = _Case(be, 256, 4, 5, 64, [64, 33, 17, 1], seed=5)
    for nstg in (3, 4):
        a, b = case.run(2, nstg, bp=0, nt=1), case.run(2, nstg, bp=0, nt=0)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), nstg


@pytest.mark.parametrize("be_name", BACKENDS)
def test_beam_stream_ignores_what_lies_behind_the_last_key(be_name):
    """Finite junk between an image's last key and the end of its stage gives the same bits as zeros there (weights exactly 0)."""
    be = get_backend(be_name)
    case = _Case(be, 128, 2, 3, 64, [37, 1, 50], seed=3)
    outs = []
    for junk in (0.0, 7.5):
        e = case.enc.copy()
        for i, n in enumerate(case.lens):
            e[i, n:] = junk
        outs.append(case.run(1, 4, bp=0, enc=e)[0])
    assert np.array_equal(outs[0], outs[1])


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("nstg,bp", [(4, 2), (3, 3)])
def test_beam_stream_dead_rows(be_name, nstg, bp):
    """live: a dead row's split partials and (m, l) are left as they were (sentinel), its live siblings' bits do not change; an image all of
    whose rows are dead is skipped."""
    be = get_backend(be_name)
    group, nsplit = 5, 2
    case = _Case(be, 256, 4, group, 64, [64, 33, 17, 1], seed=11)
    live = np.ones(case.rows, np.int32)
    live[[1, 4, 7]] = 0                      # dead rows beside live siblings (both beam subsets of image 0, the second of image 1)
    live[2 * group:3 * group] = 0            # image 2: every row dead
    sentinel = 0x7FC1
    ref = case.run(nsplit, nstg, bp=bp, part_fill=sentinel)
    got = case.run(nsplit, nstg, bp=bp, live=live, part_fill=sentinel)
    H, d, inner = case.H, case.d, case.H * 64
    part_r, part_g = ref[1].reshape(case.rows, -1), got[1].reshape(case.rows, -1)
    ml_r, ml_g = ref[2].reshape(case.rows, -1), got[2].reshape(case.rows, -1)
    sent_ml = np.float32(sentinel).view(np.uint32)
    for r in range(case.rows):
        if live[r]:
            assert np.array_equal(part_g[r], part_r[r]) and np.array_equal(ml_g[r], ml_r[r]), r
        else:
            assert np.all(part_g[r] == sentinel) and np.all(ml_g[r] == sent_ml), r
    # the contraction reads each row's own partials: live rows' contexts are the same bits
    cr = pk.unpack_tiles(ref[0], case.rows, inner).reshape(case.rows, -1)
    cg = pk.unpack_tiles(got[0], case.rows, inner).reshape(case.rows, -1)
    for r in np.nonzero(live)[0]:
        assert np.array_equal(cg[r].view(np.uint32), cr[r].view(np.uint32)), r
    assert part_r.shape == (case.rows, nsplit * H * d)


def test_beam_cross_absorb_setting_and_workspace_rule():
    """mg_set_beam_cross_absorb without device work: default 0 (K / V form); query / set return the previous value; with 1 the beam
    workspaces shrink (one buffer of states instead of per-layer K / V) while the greedy sizes stay; the greedy and beam settings are
    independent; bad values, a null model and a geometry without the absorbed form are refused."""
    from markushgrapher_amd import _lib
    from markushgrapher_amd.engine import MgConfig
    lib = _lib.load()
    lib.mg_last_error.restype = C.c_char_p
    lib.mg_set_beam_cross_absorb.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.mg_set_cross_absorb.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.mg_workspace_bytes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]
    lib.mg_stream_beam_workspace_bytes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]
    lib.mg_destroy.argtypes = [C.c_void_p]
    cfg = MgConfig(500, 64, 64, 128, 2, 2, 2, 32, 128, 128, 64, 16, 3, 0, 1, 0, 1e-6, 64)
    model = C.c_void_p()
    assert lib.mg_create(C.byref(cfg), C.byref(model)) == 0
    need = C.c_size_t()

    def ws(B, beams=1):
        assert lib.mg_workspace_bytes(model, B, 8, beams, 16, 0, 0, C.byref(need)) == 0
        return need.value

    def sws():
        assert lib.mg_stream_beam_workspace_bytes(model, 8, 8, 8, 3, 5, 16, C.byref(need)) == 0
        return need.value
    try:
        assert lib.mg_set_beam_cross_absorb(model, -1, 0) == 0             # default: the K / V form
        kv = (ws(95), ws(96), ws(32, 5), ws(3, 3), sws())
        assert lib.mg_set_beam_cross_absorb(model, 1, 3) == 0              # returns the previous setting
        assert lib.mg_set_beam_cross_absorb(model, -1, 0) == 1
        ab = (ws(95), ws(96), ws(32, 5), ws(3, 3), sws())
        assert ab[:2] == kv[:2]                                            # greedy sizes unchanged
        assert ab[2] < kv[2] and ab[3] < kv[3] and ab[4] < kv[4]           # the beam forms need less
        # independence of the two settings
        assert lib.mg_set_cross_absorb(model, -1, 0) == 2
        assert lib.mg_set_cross_absorb(model, 0, 0) == 2
        assert lib.mg_set_beam_cross_absorb(model, -1, 0) == 1 and ws(32, 5) == ab[2]
        assert lib.mg_set_beam_cross_absorb(model, 0, 0) == 1
        assert lib.mg_set_cross_absorb(model, -1, 0) == 0 and ws(32, 5) == kv[2]
        # refused
        assert lib.mg_set_beam_cross_absorb(model, 2, 0) < 0 and b"absorb" in lib.mg_last_error()
        assert lib.mg_set_beam_cross_absorb(model, 1, 5) < 0
        assert lib.mg_set_beam_cross_absorb(model, 1, -1) < 0
        assert lib.mg_set_beam_cross_absorb(None, 1, 0) < 0
        assert lib.mg_set_beam_cross_absorb(model, -1, 0) == 0             # (unchanged by the refusals)
    finally:
        lib.mg_destroy(model)
    odd = MgConfig(500, 192, 64, 128, 2, 2, 3, 32, 128, 128, 64, 16, 3, 0, 1, 0, 1e-6, 64)      # d_model 192: no absorbed form
    model = C.c_void_p()
    assert lib.mg_create(C.byref(odd), C.byref(model)) == 0
    try:
        rc = lib.mg_set_beam_cross_absorb(model, 1, 0)
        assert rc < 0 and b"no absorbed form" in lib.mg_last_error()
        assert lib.mg_set_beam_cross_absorb(model, -1, 0) == 0
    finally:
        lib.mg_destroy(model)


# ---- engine ------------------------------------------------------------------------------------------------------------------------
def _fixture(name):
    g = load_golden(name)
    shape, sd = _weights(g)
    return g, shape, sd, _inputs(g, shape)


def _args(inp):
    return inp["input_ids"], inp["bbox"], inp["attention_mask"], inp["pixel_values"]


@pytest.mark.parametrize("be_name", BACKENDS)
def test_trained_fixture_beam5_absorbed(be_name):
    """g3 (trained tiny) beam-5 with the absorbed beam form: ids bit-exact with stock, scores within 1e-2 (as the K / V form)."""
    g, shape, sd, inp = _fixture("g3_trained_tiny.npz")
    eng = make_engine(be_name, shape, sd)
    assert eng.beam_cross_absorb is False
    assert eng.set_beam_cross_absorb(True) is False and eng.beam_cross_absorb is True
    ids, scores, _ = eng.generate(*_args(inp), num_beams=5, max_length=int(g["max_length"]))
    ids, scores = eng.mem.numpy(ids), eng.mem.numpy(scores)
    assert np.array_equal(ids, g["beam_ids"]), (ids.tolist(), g["beam_ids"].tolist())
    np.testing.assert_allclose(scores, g["beam_scores"], atol=1e-2)


@pytest.mark.parametrize("be_name", BACKENDS)
def test_random_weights_beam5_absorbed(be_name):
    """g0 beam-5 under the rules of test_engine.py::test_beam_search_random_weights_scores; the scores are not the K / V form's bits
    (the new form ran)."""
    from oracle.udop_oracle import Oracle
    from tests.test_engine import _oracle_sequence_score
    g, shape, sd, inp = _fixture("g0_tiny.npz")
    eng = make_engine(be_name, shape, sd)
    T = int(g["max_length"])
    _, kv_scores, _ = eng.generate(*_args(inp), num_beams=5, max_length=T)
    kv_scores = eng.mem.numpy(kv_scores).copy()
    eng.set_beam_cross_absorb(True)
    ids, scores, _ = eng.generate(*_args(inp), num_beams=5, max_length=T)
    ids, scores = eng.mem.numpy(ids).copy(), eng.mem.numpy(scores).copy()
    assert not np.array_equal(scores.view(np.uint32), kv_scores.view(np.uint32))
    assert ids.shape == g["beam_ids"].shape and np.all(ids[:, 0] == 0)
    SCORE_TOL = 5e-2
    np.testing.assert_allclose(scores, g["beam_scores"], atol=SCORE_TOL)
    mine = _oracle_sequence_score(Oracle(shape, sd), inp, ids)
    assert np.all(mine > g["beam_scores"] - SCORE_TOL), (mine, g["beam_scores"])
    np.testing.assert_allclose(mine, scores, atol=SCORE_TOL)
    for b in range(ids.shape[0]):
        if g["beam_gap"][b] > 2 * SCORE_TOL:
            assert np.array_equal(ids[b], g["beam_ids"][b])


@pytest.mark.parametrize("be_name", BACKENDS)
def test_beam_queue_equals_per_image_calls_absorbed(be_name):
    """Under the absorbed beam form the beam queue (slots of K = 3 beams over 11 images) returns for every image the ids, length and score
    bits generate(num_beams=3) returns for it alone - as test_stream.py::test_beam_stream_equals_per_image_beam_search for the K / V form."""
    g, shape, sd, inp = _fixture("g3_trained_tiny.npz")
    K, T = 3, int(g["max_length"])
    eng = make_engine(be_name, shape, sd)
    eng.set_beam_cross_absorb(True)
    want = []
    for b in range(inp["input_ids"].shape[0]):
        one = {k: v[b:b + 1] for k, v in inp.items()}
        ids, scores, _ = eng.generate(*_args(one), num_beams=K, max_length=T)
        ids = eng.mem.numpy(ids)
        want.append((ids[0].copy(), float(eng.mem.numpy(scores)[0]), int(ids.shape[1])))
    order = np.array([0, 3, 5, 1, 2, 4, 4, 0, 1, 5, 2])
    q = {k: np.ascontiguousarray(v[order]) for k, v in inp.items()}
    ids, lens, scores, _ = eng.generate_stream_beam(*_args(q), num_beams=K, max_length=T, chunk=4, slots=3, pool_chunks=3)
    ids, lens, scores = eng.mem.numpy(ids), eng.mem.numpy(lens), eng.mem.numpy(scores)
    for n, b in enumerate(order):
        row, sc, cols = want[b]
        assert lens[n] == cols, (n, b, lens[n], cols)
        assert np.array_equal(ids[n, :cols], row[:cols]), (n, b)
        assert scores[n] == np.float32(sc), (n, b, scores[n], sc)


@pytest.mark.parametrize("be_name", BACKENDS)
def test_image_bits_independent_of_batch_mates_absorbed(be_name):
    """An image's ids and score are the same bits decoded alone and inside a 4-image call (beam-5, absorbed beam form)."""
    g, shape, sd, inp = _fixture("g3_trained_tiny.npz")
    T = int(g["max_length"])
    eng = make_engine(be_name, shape, sd)
    eng.set_beam_cross_absorb(True, key_splits=2)
    four = {k: np.ascontiguousarray(v[:4]) for k, v in inp.items()}
    ids4, sc4, _ = eng.generate(*_args(four), num_beams=5, max_length=T)
    ids4, sc4 = eng.mem.numpy(ids4).copy(), eng.mem.numpy(sc4).copy()
    for b in (0, 3):
        one = {k: v[b:b + 1] for k, v in four.items()}
        ids1, sc1, _ = eng.generate(*_args(one), num_beams=5, max_length=T)
        ids1, sc1 = eng.mem.numpy(ids1), eng.mem.numpy(sc1)
        assert np.array_equal(ids1[0], ids4[b, :ids1.shape[1]]) and sc1[0].view(np.uint32) == sc4[b].view(np.uint32), b


@pytest.mark.parametrize("be_name", BACKENDS)
def test_attached_branch_beam_absorbed(be_name):
    """With the OCSR branch e1 attached (keys = [e1 tokens | encoder states]), the absorbed beam form agrees with the K / V form: batch
    call and beam queue, scores within tolerance."""
    from tests.test_e1 import _attached
    g, shape, sd, inp, s1, sd1, eng, e1e = _attached(be_name)
    T = int(g["max_length"])
    args = _args(inp)
    _, kv, _ = eng.generate(*args, num_beams=3, max_length=T)
    kv = eng.mem.numpy(kv).copy()
    _, _, kvq, _ = eng.generate_stream_beam(*args, num_beams=3, max_length=T, chunk=4, slots=3, pool_chunks=3)
    kvq = eng.mem.numpy(kvq).copy()
    eng.set_beam_cross_absorb(True)
    _, ab, _ = eng.generate(*args, num_beams=3, max_length=T)
    ab = eng.mem.numpy(ab).copy()
    _, _, abq, _ = eng.generate_stream_beam(*args, num_beams=3, max_length=T, chunk=4, slots=3, pool_chunks=3)
    abq = eng.mem.numpy(abq).copy()
    assert np.all(np.isfinite(ab)) and np.all(np.isfinite(abq))
    np.testing.assert_allclose(ab, kv, atol=5e-2)
    np.testing.assert_allclose(abq, kvq, atol=5e-2)
    assert not np.array_equal(ab.view(np.uint32), kv.view(np.uint32))


@pytest.mark.parametrize("be_name", BACKENDS)
def test_clone_inherits_beam_setting(be_name):
    g, shape, sd, inp = _fixture("g3_trained_tiny.npz")
    eng = make_engine(be_name, shape, sd)
    assert eng.clone().beam_cross_absorb is False
    eng.set_beam_cross_absorb(True)
    c = eng.clone()
    assert c.beam_cross_absorb is True
    assert c.set_beam_cross_absorb(False) is True and eng.beam_cross_absorb is True
    ids, _, _ = eng.clone().generate(*_args(inp), num_beams=5, max_length=int(g["max_length"]))
    assert np.array_equal(eng.mem.numpy(ids), g["beam_ids"])


# ---- GPU only: the bench shape ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_g4_beam5_all_32_images_absorbed_against_stock():
    """As test_bench_config.py::test_g4_beam5_all_32_images_against_stock (32 images, 160 decode rows) with the absorbed beam form: every
    sequence score within 2 x LOGIT_TOL of stock's best, in the batch call and the beam queue; hypotheses equal to stock's best or second
    must not collapse."""
    from tests.test_bench_config import _setup, LOGIT_TOL
    g, shape, eng0, args = _setup()
    eng = eng0.clone()
    eng.set_beam_cross_absorb(True)
    gb = load_golden("g4_beam32.npz")
    new = int(gb["new_tokens"])
    ids, sc, _ = eng.generate(*args, num_beams=5, max_length=new + 1, min_length=new + 1)
    ids, sc = eng.mem.numpy(ids).copy(), eng.mem.numpy(sc).copy()
    np.testing.assert_allclose(sc, gb["beam_scores"], atol=2 * LOGIT_TOL)
    hit = sum(bool(np.array_equal(ids[b], gb["beam_ids"][b]) or np.array_equal(ids[b], gb["beam_second_ids"][b])) for b in range(ids.shape[0]))
    print(f"absorbed beam-5, batch call: {hit} of {ids.shape[0]} equal stock's best or second; max |score - stock| "
          f"{np.abs(sc - gb['beam_scores']).max():.4f}")
    assert hit >= 24, hit              # measured 27 (threshold = measured - 3)
    qi, ql, qs, _ = eng.generate_stream_beam(*args, num_beams=5, max_length=new + 1, min_length=new + 1, chunk=16, slots=16, pool_chunks=3)
    qi, ql, qs = eng.mem.numpy(qi), eng.mem.numpy(ql), eng.mem.numpy(qs)
    assert np.all(ql == new + 1)
    np.testing.assert_allclose(qs, gb["beam_scores"], atol=2 * LOGIT_TOL)
    hitq = sum(bool(np.array_equal(qi[b], gb["beam_ids"][b]) or np.array_equal(qi[b], gb["beam_second_ids"][b])) for b in range(qi.shape[0]))
    print(f"absorbed beam-5, queue form: {hitq} of {qi.shape[0]} equal stock's best or second")
    assert hitq >= 24, hitq            # measured 27 (threshold = measured - 3)


@pytest.mark.gpu
def test_beam5_max_length_512_eos_live_absorbed():
    """The reference's shipped call (beam-5, max_length 512, EOS live) on 4 bench images with the absorbed beam form: finite scores,
    lengths within 512, and the decode step replayed from its captured graph."""
    from markushgrapher_amd import synth
    from tests.test_bench_config import _setup
    g, shape, _, args = _setup()
    sd = synth.recipe_state_dict(shape, **synth.BENCH_RECIPE)
    eng = make_engine("hip", shape, sd, max_decode_len=512)
    eng.set_beam_cross_absorb(True)
    sub = tuple(a[:4] for a in args)
    ids, sc, _ = eng.generate(*sub, num_beams=5, max_length=512)
    ids, sc = eng.mem.numpy(ids), eng.mem.numpy(sc)
    assert ids.shape[0] == 4 and ids.shape[1] <= 512
    assert np.all(np.isfinite(sc))
    assert eng.decode_graph_active()


@pytest.mark.gpu
def test_model_setting_reaches_every_context():
    """MarkushgrapherForConditionalGeneration.set_beam_cross_absorb: the engine, contexts made afterwards by in_flight() and by
    generate_queue(contexts=...), and the contexts generate_queue keeps, all run the setting; turning it off reaches them too.  The beam
    queue on two contexts returns the per-image beam calls' ids under the absorbed form.  (The model refuses a CPU device, hence GPU only.)"""
    import torch
    from tests.test_modeling import tiny_model
    m, shape = tiny_model()
    m = m.to("cuda")
    assert m.set_beam_cross_absorb(True) is False
    assert m._eng().beam_cross_absorb is True
    with m.in_flight(3) as fl:
        assert all(c.beam_cross_absorb for c in fl.contexts)
    g = load_golden("g3_trained_tiny.npz")
    encodings = [{"input_ids": torch.from_numpy(g["input_ids"][k:k + 1]), "bbox": torch.from_numpy(g["bbox"][k:k + 1]),
                  "pixel_values": torch.from_numpy(g["pixel_values"][k:k + 1])} for k in range(6)]
    loop = []
    for e in encodings:
        enc = {k: v.to(m.device) for k, v in e.items()}
        loop.append(m.generate(**enc, num_beams=3, max_length=16)[0].cpu().tolist())
    got = m.generate_queue(encodings, max_length=16, slots=3, chunk=2, num_beams=3, contexts=2)
    assert len(m._inflight.contexts) == 2 and all(c.beam_cross_absorb for c in m._inflight.contexts)
    for a, b in zip(got, loop):
        a = a.cpu().tolist()
        assert a == b[:len(a)] and len(a) >= 2, (a, b)
    assert m.set_beam_cross_absorb(False) is True
    assert not m._eng().beam_cross_absorb and not any(c.beam_cross_absorb for c in m._inflight.contexts)
