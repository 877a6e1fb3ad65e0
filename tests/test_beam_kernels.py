"""The device beam step (k_beam.hip) driven step by step on scripted logits (tests/beam_script.py) through the mgk_beam_* hooks,
against the float64 stock restatement: ids, beam indices and the continue flag exactly at every step, the ancestor table after every
step, the n-best outputs exactly and the scores within float32 accumulation bounds; both position forms bit for bit; the queue form per
image bit for bit against the batch form."""
import ctypes as C

import numpy as np
import pytest

from tests.backends import get_backend
from tests.beam_script import Script, reference, tie_free

EOS, START = 7, 1
NAN_PAD = np.float32(np.nan)


def _lib(be):
    lib = be.lib
    lib.mgk_beam_state_bytes.restype = C.c_size_t
    lib.mgk_beam_length_divisor.restype = C.c_float
    lib.mgk_beam_length_divisor.argtypes = [C.c_int, C.c_float]
    return lib


class Logits:
    """[rows][ldl] float32 logits on the device; columns >= V poisoned once, each step rewrites only the rows' first V columns."""

    def __init__(self, be, rows, V, ldl, poison):
        self.be, self.V = be, V
        self.host = np.full((rows, ldl), poison, np.float32)
        self.dev = be.buf(self.host)

    def set(self, rows):
        for r, row in rows.items():
            self.host[r, :self.V] = row
        if self.be.name == "emu":
            self.dev.a[...] = self.host
        else:
            import torch
            self.dev.a.copy_(torch.from_numpy(self.host))


def _read(be, buf):
    return buf.numpy().copy()


def _write(be, buf, arr):
    if be.name == "emu":
        buf.a[...] = arr
    else:
        import torch
        buf.a.copy_(torch.from_numpy(np.ascontiguousarray(arr)))


def run_batch(be, script, B, K, max_length, ldl=None, poison=NAN_PAD, min_length=0, length_penalty=1.0, early_stopping=False, num_return=1,
              pad=0, dev_pos=False, ref=None):
    """The batch form as mg_generate enqueues it; checked against `ref` (a reference() result) at every step when given."""
    lib = _lib(be)
    V, R = script.V, B * K
    ldl = ldl or V
    T_cap = max_length - 1
    state = be.zeros(lib.mgk_beam_state_bytes(B, K, max_length), np.uint8)
    nid, bidx, ctr = be.zeros(R, np.int64), be.zeros(R, np.int32), be.zeros(8, np.int32)
    anc = be.zeros((T_cap, R), np.int32)
    div = be.buf(np.array([lib.mgk_beam_length_divisor(c, length_penalty) for c in range(max_length + 1)], np.float32))
    tdev = be.zeros(1, np.int32)
    lg = Logits(be, R, V, ldl, poison)
    s = be.stream
    assert lib.mgk_beam_init(s, be.p(state), B, K, max_length, pad, EOS, START, be.p(nid), be.p(anc), T_cap, be.p(ctr)) == 0
    prefixes = [[START] for _ in range(R)]
    anc_ref = np.tile(np.arange(R, dtype=np.int32), (T_cap, 1))
    steps = []
    for t in range(max_length - 1):
        lg.set({r: script.logits(r // K, prefixes[r]) for r in range(R)})
        if dev_pos:
            _write(be, tdev, np.array([t], np.int32))
        assert lib.mgk_beam_step(s, be.p(state), be.p(lg.dev), ldl, V, B, K, max_length, t + 1, be.p(tdev) if dev_pos else None,
                                 be.p(div), EOS, min_length, C.c_float(length_penalty), int(early_stopping), be.p(nid), be.p(bidx),
                                 be.p(ctr), None, None) == 0
        assert lib.mgk_beam_reorder_anc(s, be.p(anc), be.p(bidx), R, max_length - 1 if dev_pos else t + 1, be.p(tdev) if dev_pos else None,
                                        be.p(ctr), None, None) == 0
        n, bi, cont = _read(be, nid), _read(be, bidx), bool(_read(be, ctr)[0])
        steps.append(dict(next_ids=n, beam_idx=bi, cont=cont))
        if ref is not None:
            assert t < len(ref["steps"]), "the kernel ran more steps than the reference"
            rs = ref["steps"][t]
            assert np.array_equal(n, rs["next_ids"]), ("next_ids", t)
            assert np.array_equal(bi, rs["beam_idx"]), ("beam_idx", t)
            assert cont == rs["cont"], ("continue flag", t)
        if cont:            # the reorder runs while the batch continues, over the written positions j <= t
            anc_ref[:t + 1] = anc_ref[:t + 1][:, bi]
        assert np.array_equal(_read(be, anc), anc_ref), ("ancestor table", t)
        prefixes = [prefixes[bi[r]] + [int(n[r])] for r in range(R)]
        if not cont:
            break
    nr = num_return
    out_ids, out_cols, out_sc = be.zeros((B * nr, max_length), np.int64), be.zeros(1, np.int32), be.zeros(B * nr, np.float32)
    obi, ots = be.zeros((B * nr, max_length - 1), np.int32), be.zeros((B * nr, max_length - 1), np.float32)
    assert lib.mgk_beam_finalize(s, be.p(state), B, K, max_length, be.p(out_ids), be.p(out_cols), be.p(out_sc), nr, be.p(obi), be.p(ots)) == 0
    return dict(steps=steps, out_ids=_read(be, out_ids), cols=int(_read(be, out_cols)[0]), scores=_read(be, out_sc),
                beam_indices=_read(be, obi), token_scores=_read(be, ots), state=_read(be, state), anc=_read(be, anc))


def check_outputs(out, ref, max_length, n_steps_bound):
    """n-best against the reference: ids / beam indices exact; scores within float32 accumulation over the run."""
    seq = ref["sequences"]
    n = seq.shape[1] - 1
    assert len(out["steps"]) == len(ref["steps"]), "steps run"
    assert out["cols"] == 1 + n
    assert np.array_equal(out["out_ids"][:, :1 + n], seq)
    assert np.array_equal(out["beam_indices"][:, :n], ref["beam_indices"])
    assert (out["beam_indices"][:, n:] == -1).all() and (out["token_scores"][:, n:] == 0).all()
    # a token score is one float32 log-softmax of |x - max| <= 2e4 (+-1e4 rows): 2 ulp of the operands; a sequence score is a float32
    # running sum of n_steps of them (one rounding each) divided once: n_steps * ulp(|score|) + the token errors
    tok_tol = 4e-3 if np.abs(ref["token_scores"]).max() > 1e3 else 2e-5
    np.testing.assert_allclose(out["token_scores"][:, :n], ref["token_scores"], rtol=0, atol=tok_tol)
    sc = np.abs(ref["scores"]).max()
    np.testing.assert_allclose(out["scores"], ref["scores"], rtol=0, atol=n_steps_bound * (np.spacing(np.float32(sc)) + tok_tol))


def _case(be_name, script_kw, B, K, max_length, ldl_extra=37, **o):
    be = get_backend(be_name)
    if script_kw.get("kind", "soft") == "soft":
        script, ref = tie_free(lambda seed: Script(seed=seed, **script_kw), lambda sc: reference(sc, B, K, max_length, start=START, **o))
    else:
        script = Script(**script_kw)
        ref = reference(script, B, K, max_length, start=START, **o)
    out = run_batch(be, script, B, K, max_length, ldl=script.V + ldl_extra, ref=ref, **o)
    check_outputs(out, ref, max_length, len(ref["steps"]))
    return be, script, ref, out


def er_mid(image, cur_len):
    return 2 if (image + cur_len) % 3 == 0 else (6 if (image + cur_len) % 4 == 1 else None)


# ---- the CPU tier: small vocabularies, a few images, a few dozen steps ----------------------------------------------------------

SMALL = [
    # (script, B, K, max_length, options)
    (dict(V=500, eos=EOS, eos_rank=er_mid), 3, 5, 20, dict(length_penalty=0.7, num_return=2)),
    (dict(V=500, eos=EOS, eos_rank=er_mid), 2, 2, 24, dict(early_stopping=True, num_return=2, min_length=5)),
    (dict(V=520, eos=EOS, eos_rank=er_mid), 2, 8, 16, dict(length_penalty=0.7, num_return=8, pad=3, min_length=4)),
    (dict(V=500, eos=EOS, eos_rank=er_mid), 3, 5, 30, dict(min_length=10, length_penalty=-0.5)),
    (dict(V=500, eos=EOS, eos_rank=er_mid), 2, 5, 2, dict()),                                                    # every candidate hits
    # exact ties: duplicated values in a row, identical rows across beams (equal running scores), uniform rows, large magnitudes
    (dict(V=500, eos=EOS, kind="grid", seed=3, dup=6, same_rows=True, eos_rank=er_mid), 2, 5, 24, dict(num_return=5)),
    (dict(V=300, eos=EOS, kind="grid", seed=4, n_hot=6, uniform_every=3, eos_rank=er_mid), 2, 5, 18, dict(length_penalty=0.0, num_return=5)),
    (dict(V=500, eos=EOS, kind="grid", seed=5, big=1.0e4, dup=3, eos_rank=er_mid), 2, 5, 20, dict(num_return=2, early_stopping=True)),
]


@pytest.mark.parametrize("case", SMALL)
def test_batch_step_matches_reference_emu(case):
    script_kw, B, K, ml, o = case
    _case("emu", script_kw, B, K, ml, **o)


def eos_k_to_2k(image, cur_len):
    """step 1: EOS is row 0's candidate K + 1 (a hit that must not finish); later steps: inside the top K for image 1 only"""
    if cur_len == 1:
        return 6
    return 1 if image == 1 and cur_len % 4 == 0 else None


def test_eos_between_k_and_2k_hits_but_does_not_finish_emu():
    be, script, ref, out = _case("emu", dict(V=400, eos=EOS, kind="grid", seed=9, eos_rank=eos_k_to_2k), 2, 5, 12, num_return=5)
    # step 1: EOS is candidate 5 of image 0 (row rank 6): not among the running beams, not a finished hypothesis
    assert EOS not in out["steps"][0]["next_ids"][:5]
    assert not any(row[1] == EOS for row in out["out_ids"][:5])


def test_eos_suppressed_by_min_length_emu():
    # EOS is every row's top token; min_length keeps it out until cur_len = 6, then the first finished hypotheses end there
    be, script, ref, out = _case("emu", dict(V=300, eos=EOS, kind="grid", seed=2, eos_rank=lambda i, c: 1), 2, 5, 16, min_length=6,
                                 num_return=5)
    for s in out["steps"][:5]:
        assert EOS not in s["next_ids"]
    assert (out["out_ids"][:, 6] == EOS).any()


def test_stopped_image_stays_frozen_emu():
    """image 0: EOS is every row's top token, so all its beams finish by step 2 and its heuristic stops it; image 1 goes on.  With
    length penalty 2 image 0's later EOS candidates would outscore its worst finished one: the heuristic gate must keep them out."""
    be, script, ref, out = _case("emu", dict(V=300, eos=EOS, kind="grid", seed=6, eos_rank=lambda i, c: 1 if i == 0 else None), 2, 5, 10,
                                 length_penalty=2.0, num_return=5)
    assert len(out["steps"]) == 9
    assert out["beam_indices"][:5, 2:].max() == -1        # image 0's hypotheses all ended by step 2


@pytest.mark.parametrize("V", [33201, 40961])
def test_product_and_generic_vocab_few_steps_emu(V):
    """the register path at the product vocabulary and the generic loop beyond 40960 columns, poisoned padding (NaN)"""
    _case("emu", dict(V=V, eos=EOS, eos_rank=er_mid, n_hot=16), 1, 2, 4, ldl_extra=63)


def test_huge_padding_never_read_emu():
    _case("emu", dict(V=40960, eos=EOS, eos_rank=er_mid, n_hot=16), 1, 2, 3, ldl_extra=64)
    be = get_backend("emu")
    script = Script(V=600, eos=EOS, kind="grid", seed=1, eos_rank=er_mid)
    ref = reference(script, 2, 5, 10, start=START)
    out = run_batch(be, script, 2, 5, 10, ldl=640, poison=np.float32(3.0e38), ref=ref)
    check_outputs(out, ref, 10, len(ref["steps"]))


def test_position_forms_bit_identical_emu():
    be = get_backend("emu")
    script = Script(V=500, eos=EOS, kind="grid", seed=7, dup=4, eos_rank=er_mid)
    o = dict(length_penalty=0.7, early_stopping=True, num_return=3, min_length=3)
    ref = reference(script, 3, 5, 20, start=START, **o)
    a = run_batch(be, script, 3, 5, 20, ldl=512, ref=ref, **o)
    b = run_batch(be, script, 3, 5, 20, ldl=512, ref=ref, dev_pos=True, **o)
    check_outputs(a, ref, 20, len(ref["steps"]))
    for k in ("out_ids", "scores", "beam_indices", "token_scores", "state", "anc"):
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    assert a["cols"] == b["cols"]


def run_queue(be, script, N, slots, K, max_length, ready, min_length=0, length_penalty=1.0, early_stopping=False, num_return=1, pad=0):
    """The queue form as mg_generate_stream_beam enqueues a step: beam_step (slots) -> reorder (slots) -> slots_step(end first).
    ready(step) = images available to the slots before that step.  The ancestor table is checked after every step."""
    lib = _lib(be)
    V, R = script.V, slots * K
    T_cap = max_length - 1
    state = be.zeros(lib.mgk_beam_state_bytes(slots, K, max_length), np.uint8)
    pos, img, pool, live = be.zeros(R, np.int32), be.buf(np.full(R, -1, np.int32)), be.zeros(R, np.int32), be.zeros(R, np.int32)
    bpool, assign = be.zeros(slots, np.int32), be.buf(np.full(slots, -1, np.int32))
    nid, bidx, ctr = be.buf(np.full(R, START, np.int64)), be.zeros(R, np.int32), be.zeros(16, np.int32)
    anc = be.zeros((T_cap, R), np.int32)
    nr = num_return
    out_ids = be.buf(np.full((N * nr, max_length), pad, np.int64))
    out_len, out_sc = be.zeros(N, np.int32), be.zeros(N * nr, np.float32)
    obi, ots = be.zeros((N * nr, max_length - 1), np.int32), be.zeros((N * nr, max_length - 1), np.float32)
    div = be.buf(np.array([lib.mgk_beam_length_divisor(c, length_penalty) for c in range(max_length + 1)], np.float32))
    lg = Logits(be, R, V, V + 29, NAN_PAD)
    s = be.stream
    prefixes = [None] * R
    anc_ref = _read(be, anc)
    h_live, h_img, h_pos = np.zeros(R, np.int32), np.full(R, -1, np.int32), np.zeros(R, np.int32)
    ends = {}
    for step in range(N * max_length + 8):
        c = _read(be, ctr)
        c[5] = ready(step)
        _write(be, ctr, c)
        lg.set({r: script.logits(int(h_img[r]), prefixes[r]) for r in range(R) if h_live[r]})
        assert lib.mgk_beam_step(s, be.p(state), be.p(lg.dev), V + 29, V, slots, K, max_length, 0, None, be.p(div), EOS, min_length,
                                 C.c_float(length_penalty), int(early_stopping), be.p(nid), be.p(bidx), be.p(ctr), be.p(pos), be.p(live)) == 0
        assert lib.mgk_beam_reorder_anc(s, be.p(anc), be.p(bidx), R, max_length - 1, None, be.p(ctr), be.p(pos), be.p(live)) == 0
        assert lib.mgk_beam_slots_step(s, be.p(state), slots, K, max_length, pad, EOS, START, int(early_stopping), be.p(pos), be.p(img),
                                       be.p(pool), be.p(bpool), be.p(live), be.p(assign), be.p(nid), be.p(anc), T_cap, 4, be.p(out_ids),
                                       be.p(out_len), be.p(out_sc), be.p(ctr), 1, nr, be.p(obi), be.p(ots)) == 0
        n, bi = _read(be, nid), _read(be, bidx)
        p_live, p_img, p_pos = _read(be, live), _read(be, img), _read(be, pos)
        # ancestors: rows of slots live during the step are permuted at the positions they have written (j <= pos); newly assigned
        # slots restart from the identity
        new = anc_ref.copy()
        for r in range(R):
            if h_live[r]:
                new[:h_pos[r] + 1, r] = anc_ref[:h_pos[r] + 1, bi[r]]
        for r in range(R):
            if p_live[r] and not (h_live[r] and p_img[r] == h_img[r]):
                new[:, r] = r
        anc_ref = new
        now = _read(be, anc)
        live_rows = [r for r in range(R) if p_live[r]]
        assert np.array_equal(now[:, live_rows], anc_ref[:, live_rows]), ("ancestor table", step)
        anc_ref = now        # (rows of idle slots are not specified)
        old = prefixes
        prefixes = [None] * R
        for r in range(R):
            if p_live[r] and h_live[r] and p_img[r] == h_img[r]:
                prefixes[r] = old[bi[r]] + [int(n[r])]
            elif p_live[r]:
                prefixes[r] = [START]
                assert n[r] == START
        for r in range(0, R, K):
            if h_live[r] and not (p_live[r] and p_img[r] == h_img[r]):
                ends[int(h_img[r])] = step
        h_live, h_img, h_pos = p_live, p_img, p_pos
        if _read(be, ctr)[1] == N:
            break
    return dict(out_ids=_read(be, out_ids), out_len=_read(be, out_len), scores=_read(be, out_sc), beam_indices=_read(be, obi),
                token_scores=_read(be, ots), ends=ends)


def check_queue(q, batch, ref, N, nr):
    assert len(q["ends"]) == N
    for i in range(N):
        rows = slice(i * nr, (i + 1) * nr)
        assert np.array_equal(q["out_ids"][rows], batch["out_ids"][rows]), ("ids", i)
        assert np.array_equal(q["beam_indices"][rows], batch["beam_indices"][rows]), ("beam indices", i)
        assert np.array_equal(q["scores"][rows].view(np.uint32), batch["scores"][rows].view(np.uint32)), ("scores", i)
        assert np.array_equal(q["token_scores"][rows].view(np.uint32), batch["token_scores"][rows].view(np.uint32)), ("token scores", i)
        n_i = int((ref["beam_indices"][rows] != -1).sum(axis=1).max())
        assert q["out_len"][i] == 1 + n_i


def test_queue_form_matches_batch_form_emu():
    """5 images through 2 slots, entering as they become ready; early stopping ends images at different steps"""
    be = get_backend("emu")
    N, K, ml, nr = 5, 5, 24, 2
    script = Script(V=400, eos=EOS, kind="grid", seed=11, dup=2, eos_rank=lambda i, c: 1 if (c + i) % (3 + i) == 0 else (7 if c % 2 else None))
    o = dict(early_stopping=True, num_return=nr, length_penalty=0.7)
    ref = reference(script, N, K, ml, start=START, **o)
    batch = run_batch(be, script, N, K, ml, ldl=432, ref=ref, **o)
    check_outputs(batch, ref, ml, len(ref["steps"]))
    q = run_queue(be, script, N, 2, K, ml, ready=lambda step: min(N, 1 + step // 3), **o)
    check_queue(q, batch, ref, N, nr)
    assert len(set(q["ends"].values())) > 2, q["ends"]


# ---- the GPU tier: the bench geometry, the long run, the generic loop at B * K = 256 ----------------------------------------------

def er_long(image, cur_len):
    """EOS at rank 2 or 3 of some rows all along, at rank 1 for a few images late in the run"""
    if image % 8 == 3 and cur_len > 300 + image:
        return 1
    return 2 + (image + cur_len) % 2 if (image * 7 + cur_len) % 11 == 0 else None


@pytest.mark.gpu
def test_bench_geometry_512_steps_hip():
    """B = 32, K = 5, V = 33201, max_length = 512, EOS live, in the captured graph's position form (tdev + divisor table).  Length penalty
    0: over 500 steps, finished scores divided by different lengths come closer than the reference's 1e-3 margin."""
    be = get_backend("hip")
    script = Script(V=33201, eos=EOS, kind="grid", seed=21, dup=3, eos_rank=er_long)
    ref = reference(script, 32, 5, 512, start=START, num_return=2, length_penalty=0.0)
    assert len(ref["steps"]) > 400
    out = run_batch(be, script, 32, 5, 512, ldl=33216, ref=ref, num_return=2, length_penalty=0.0, dev_pos=True)
    check_outputs(out, ref, 512, len(ref["steps"]))


@pytest.mark.gpu
@pytest.mark.parametrize("V", [40960, 40961, 50000])
def test_wide_vocab_256_rows_hip(V):
    be = get_backend("hip")
    script = Script(V=V, eos=EOS, kind="grid", seed=V, dup=5, eos_rank=er_mid)
    o = dict(length_penalty=0.7, early_stopping=True, num_return=8, min_length=3)
    ref = reference(script, 32, 8, 12, start=START, **o)
    out = run_batch(be, script, 32, 8, 12, ldl=V + 96, ref=ref, **o)
    check_outputs(out, ref, 12, len(ref["steps"]))


@pytest.mark.gpu
@pytest.mark.parametrize("case", SMALL[:6])
def test_batch_step_matches_reference_hip(case):
    script_kw, B, K, ml, o = case
    _case("hip", script_kw, B, K, ml, **o)


@pytest.mark.gpu
def test_queue_form_product_vocab_hip():
    """12 images through 5 slots at the product vocabulary; images end at different steps"""
    be = get_backend("hip")
    N, K, ml, nr = 12, 5, 40, 5
    script = Script(V=33201, eos=EOS, kind="grid", seed=13, dup=2, eos_rank=lambda i, c: 1 if (c + i) % (5 + i % 7) == 0 else None)
    o = dict(early_stopping=True, num_return=nr)
    ref = reference(script, N, K, ml, start=START, **o)
    batch = run_batch(be, script, N, K, ml, ldl=33216, ref=ref, **o)
    check_outputs(batch, ref, ml, len(ref["steps"]))
    q = run_queue(be, script, N, 5, K, ml, ready=lambda step: min(N, 3 + step // 2), **o)
    check_queue(q, batch, ref, N, nr)
    assert len(set(q["ends"].values())) > 4, q["ends"]
