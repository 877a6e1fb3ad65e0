"""The single-query attention of the decode step (attn_step_kernel, k_decode.hip) in the forms the engine launches it in, and the online
softmax of the weight-absorbed stream (k_xattn.hip) under score profiles that stress it.

Reference: plain numpy float64 softmax attention on the bf16-rounded operands, one function per form (ref_self, ref_cross, ref_rope).
Tolerance: the project's bound for the step kernel (probabilities and sums in fp32, output rounded to bf16), rtol = 1/128 and
atol = 2e-3 scaled by max|V| of the case.

Every case first checks ON THE REFERENCES ALONE that its inputs can tell a subtly wrong kernel from a right one: the float64 result of
a kernel that drops one key (the last key; the first key of the second 128-key round), that looks the bias up one distance off, or
that reads the neighbouring head / row / owner / scale must differ from the true reference by more than 4 x the tolerance.  Random
scores cannot do that over hundreds of keys (one key weighs 1/n), so the boundary keys are made heavy: key vector c*e_0 against
queries with q[0] = 2, c chosen so that the boundary keys together hold at least 80 % of the softmax weight (each at least a quarter).
"""
import ctypes as C

import numpy as np
import pytest

from tests import pkutil as pk
from tests.backends import get_backend

BACKENDS = [pytest.param("emu"), pytest.param("hip", marks=pytest.mark.gpu)]
RTOL, ATOL = 1.0 / 128, 2e-3
SENT = 0xBEEF            # bf16 bit pattern (-0.4668) that no launch may leave outside its window
ROUND = 128              # keys per round of the step kernel: 8 key slots x U loads x NW waves, in both shipped forms


def ci(x):
    return C.c_int(int(x))


def cf(x):
    return C.c_float(float(x))


def P(be, b):
    return be.p(b) if b is not None else None


def ibuf(be, a):
    return None if a is None else be.buf(np.asarray(a, np.int32))


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 references
# ---------------------------------------------------------------------------------------------------------------------------------
def attend(s, V, drop=None):
    """softmax(s) @ V in float64; `drop`: indices of keys a wrong kernel leaves out (nothing left: zeros)."""
    s, V = np.asarray(s, np.float64), np.asarray(V, np.float64)
    if drop is not None:
        keep = np.ones(len(s), bool)
        keep[list(drop)] = False
        s, V = s[keep], V[keep]
    if len(s) == 0:
        return np.zeros(V.shape[1])
    p = np.exp(s - s.max())
    return (p / p.sum()) @ V


def weights(s):
    p = np.exp(np.asarray(s, np.float64) - np.max(s))
    return p / p.sum()


def lse(s):
    if len(s) == 0:
        return -np.inf
    m = np.max(s)
    return m + np.log(np.exp(s - m).sum())


def self_scores(q, K, bias_h, t, shift=0):
    """decoder self-attention: keys [0, t], bias by distance t - j (`shift`: a wrong kernel's off-by-one distance)"""
    n = t + 1
    s = np.asarray(K[:n], np.float64) @ np.asarray(q, np.float64)
    if bias_h is not None:
        s = s + np.asarray(bias_h, np.float64)[np.clip(t - np.arange(n) + shift, 0, len(bias_h) - 1)]
    return s


def ref_self(q, K, V, bias_h, t, drop=None, shift=0):
    return attend(self_scores(q, K, bias_h, t, shift), V[:t + 1], drop)


def cross_scores(q, K, n, r):
    """cross-attention: the owner's n keys, no bias, scores times the deferred RMSNorm scale r of the query row"""
    return (np.asarray(K[:n], np.float64) @ np.asarray(q, np.float64)) * r


def ref_cross(q, K, V, n, r=1.0, drop=None):
    return attend(cross_scores(q, K, n, r), V[:n], drop)


def row_scale(part, inv_d, eps):
    return 1.0 / np.sqrt(np.asarray(part, np.float64).sum(-1) * inv_d + eps)


def rope_table(positions, theta=10000.0):
    """[pos][cos 32 | sin 32], computed in float64 and stored fp32 (inv_freq_i = theta^(-i/32), as modeling_llama.py)"""
    ang = np.arange(positions, dtype=np.float64)[:, None] * theta ** (-np.arange(32, dtype=np.float64) / 32.0)[None]
    return np.concatenate([np.cos(ang), np.sin(ang)], 1).astype(np.float32)


def rotate(x, cs_row):
    """x*cos + rotate_half(x)*sin with rotate_half(x) = [-x[32:], x[:32]]: dims j and j + 32 pair up"""
    x = np.asarray(x, np.float64)
    cs_row = np.asarray(cs_row, np.float64)
    cos, sin = np.concatenate([cs_row[:32]] * 2), np.concatenate([cs_row[32:]] * 2)
    return x * cos + np.concatenate([-x[32:], x[:32]]) * sin


def rope_new(row, G, Hkv, h, cs_row, r, qscale):
    """exact (float64, unrounded) q heads of key/value head h, new k and new v of one fp32 row [G*Hkv q | Hkv k | Hkv v] x 64"""
    row = np.asarray(row, np.float64)
    Hq = G * Hkv
    qs = [rotate(row[(h * G + g) * 64:(h * G + g + 1) * 64] * r, cs_row) * qscale for g in range(G)]
    k = rotate(row[(Hq + h) * 64:(Hq + h + 1) * 64] * r, cs_row)
    v = row[(Hq + Hkv + h) * 64:(Hq + Hkv + h + 1) * 64] * r
    return qs, k, v


def ref_rope(row, G, Hkv, h, t, cs_row, r, qscale, Kc, Vc, drop=None):
    """rotary grouped-query step: q*r*rot*qscale, k*r*rot, v*r rounded to bf16, keys = cache [0, t) + the new one.  -> [G][64], k, v"""
    qs, k, v = rope_new(row, G, Hkv, h, cs_row, r, qscale)
    kb, vb = pk.bf16_round(k).astype(np.float64), pk.bf16_round(v).astype(np.float64)
    K = np.concatenate([np.asarray(Kc[:t], np.float64), kb[None]])
    V = np.concatenate([np.asarray(Vc[:t], np.float64), vb[None]])
    out = [attend(K @ pk.bf16_round(qg).astype(np.float64), V, drop) for qg in qs]
    return np.stack(out), k, v


# ---------------------------------------------------------------------------------------------------------------------------------
# tolerance and the check that the inputs discriminate
# ---------------------------------------------------------------------------------------------------------------------------------
def tol_of(ref, vmax):
    return RTOL * np.abs(ref) + ATOL * vmax


def assert_close(got, ref, vmax, what):
    err, tol = np.abs(np.asarray(got, np.float64) - ref), tol_of(ref, vmax)
    bad = err > tol
    assert not bad.any(), (what, "worst error / tolerance", float((err / tol).max()), "at", np.argwhere(bad)[:4].tolist(),
                           "max abs error", float(err.max()))


def bites(ref, mutant, vmax):
    """the wrong kernel's result is further than 4 x the tolerance from the reference somewhere"""
    return bool((np.abs(mutant - ref) > 4.0 * tol_of(ref, vmax)).any())


def profiles(n, R):
    """Score streams that stress an online softmax over n keys consumed R at a time.  Every value is a multiple of 0.5 below 128 or a
    multiple of 4 below 1024 in magnitude: exact in bf16, so that q = e_0 against keys s_j*e_0 gives exactly these scores."""
    j = np.arange(n)
    out = {"rise": 4.0 * (j - n // 2), "fall": -4.0 * (j - n // 2), "equal": np.zeros(n)}
    # XA_DEFER edge of the absorbed stream: the maximum rises per 16-key stage by 5.5 (7.93 log2 units: just under 8), later by 6.0 (8.66)
    nst = (n + 15) // 16
    stage = np.concatenate([[0.0], np.cumsum(np.where(np.arange(1, nst) <= nst // 2, 5.5, 6.0))])
    out["defer"] = stage[j // 16]
    assert np.abs(out["rise"]).max() <= 1024 and out["defer"].max() < 128
    tail = (n - 1) // R * R
    for name, p in (("first", 0), ("last", n - 1), ("round_end", R - 1), ("round_start", R), ("tail", tail + (n - tail) // 2)):
        s = np.zeros(n)
        s[p] = 60.0          # one key 60 units above the rest
        out["spike_" + name] = s
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# launching
# ---------------------------------------------------------------------------------------------------------------------------------
def new_ctx(be, rows, ld):
    """packed context buffer of ld columns, rows padded to 32 plus one spare row tile, filled with the sentinel"""
    return be.buf(np.full((((rows + 31) // 32 * 32 + 32) * ld,), SENT, np.uint16))


def read_ctx(ctx, rows, width, ld, col0, dead=()):
    """bits [rows][width] of the window; everything outside it, every row >= rows and every dead row must still hold the sentinel"""
    bits = np.array(ctx.numpy(), copy=True)
    Rp = bits.size // ld
    nat = np.ascontiguousarray(bits.reshape(Rp // 32, ld // 16, 2, 32, 8).transpose(0, 3, 1, 2, 4)).reshape(Rp, ld)
    untouched = np.ones((Rp, ld), bool)
    untouched[:rows, col0:col0 + width] = False
    untouched[list(dead)] = True
    assert (nat[untouched] == SENT).all(), ("written outside the window / past the rows / in a dead row", np.argwhere(untouched & (nat != SENT))[:6].tolist())
    return nat[:rows, col0:col0 + width].copy()


def step_ex(be, q, Kc, Vc, ctx, rows, H, group, cap, lens=None, n_keys=0, bias=None, anc=None, t=0, t_dev=None, t_off=0, pos_rows=None,
            kv_owner=None, live=None, qrs=None, inv_d=0.0, eps=0.0, ctx_ld=0, ctx_col0=0, one_wg_per_cu=0):
    nparts = 0 if qrs is None else qrs.shape[-1]
    rc = be.lib.mgk_attention_step_ex(be.stream, P(be, q), P(be, Kc), P(be, Vc), P(be, ctx), ci(rows), ci(H), ci(group), ci(cap), P(be, lens),
                                      ci(n_keys), P(be, bias), P(be, anc), ci(t), P(be, t_dev), ci(t_off), P(be, pos_rows), P(be, kv_owner),
                                      P(be, live), P(be, qrs), ci(nparts), cf(inv_d), cf(eps), ci(ctx_ld), ci(ctx_col0), ci(one_wg_per_cu))
    assert rc == 0, rc


def step_rope(be, qkv, ld, cs, rs, inv_d, eps, qscale, Kc, Vc, ctx, rows, Hkv, G, cap, t=0, t_dev=None, t_off=0, pos_rows=None,
              t_off_rows=None, kv_owner=None, live=None, ctx_ld=0, ctx_col0=0):
    nparts = 0 if rs is None else rs.shape[-1]
    return be.lib.mgk_attention_step_rope(be.stream, P(be, qkv), ci(ld), P(be, cs), P(be, rs), ci(nparts), cf(inv_d), cf(eps), cf(qscale),
                                          P(be, Kc), P(be, Vc), P(be, ctx), ci(rows), ci(Hkv), ci(G), ci(cap), ci(t), P(be, t_dev), ci(t_off),
                                          P(be, pos_rows), P(be, t_off_rows), P(be, kv_owner), P(be, live), ci(ctx_ld), ci(ctx_col0))


def bf(be, x):
    return be.buf(pk.bf16_bits(x))


def b16(x):
    return float(pk.bf16_round(np.array([x], np.float32))[0])


def bf16_exact_up(c, step=0.25):
    return float(np.ceil(c / step) * step)


# ---------------------------------------------------------------------------------------------------------------------------------
# a. key-count sweep of the self form (8 waves), three deliveries of the position; d. the context window
# ---------------------------------------------------------------------------------------------------------------------------------
SWEEP = list(range(259)) + [382, 383, 384, 385, 386, 510, 511]
SAME_BITS = (0, 1, 127, 128, 129, 511)


def self_inputs(positions, H, cap, seed):
    """per row its own cache and position; heavy keys: the last one (t) and, past it, the first of the second round (128)"""
    rs = np.random.RandomState(seed)
    rows = len(positions)
    q = pk.bf16_round(rs.standard_normal((rows, H, 64)) * 0.5)
    q[:, :, 0] = 2.0
    K = pk.bf16_round(rs.standard_normal((rows, H, cap, 64)) * 0.5)
    V = pk.bf16_round(rs.standard_normal((rows, H, cap, 64)) * 0.5)
    bias = (rs.standard_normal((cap, H)) * 2.0).astype(np.float32)       # comparable to the scores (std 2.2)
    heavy = []
    for r, t in enumerate(positions):
        hv = [t] + ([ROUND] if t > ROUND else [])
        heavy.append(hv)
        for h in range(H):
            s = self_scores(q[r, h], K[r, h], bias[:, h], t)
            # the heavy keys together hold 80 %: the rest stays heavy enough for a wrong bias distance to show
            target = lse(np.delete(s, hv)) + np.log(4.0) if len(s) > len(hv) else 4.0
            for j in hv:
                K[r, h, j] = 0.0
                K[r, h, j, 0] = b16((target - float(bias[t - j, h])) / 2.0)
    return q, K, V, bias, heavy


@pytest.mark.parametrize("be_name", BACKENDS)
def test_self_form_key_count_sweep(be_name):
    """Every position 0..258, 382..386, 510, 511 (capacity 512, H = 2) through pos_rows, several rows per launch, with a random bias
    table and the context written as the middle third of a 3*H*64 wide buffer.  For 0, 1, 127, 128, 129, 511 the same row is also run
    with the position passed by the host and through t_dev + t_off: same bits."""
    be = get_backend(be_name)
    H, cap = 2, 512
    q, K, V, bias, heavy = self_inputs(SWEEP, H, cap, 1001)
    rows, vmax = len(SWEEP), float(np.abs(V).max())
    ref = np.zeros((rows, H, 64))
    for r, t in enumerate(SWEEP):
        nb = (r + 1) % rows
        seen = dict(last=False, second=t < ROUND, bias=t == 0, head=False, row=False)      # (one key: the softmax is 1 whatever the bias)
        for h in range(H):
            ref[r, h] = ref_self(q[r, h], K[r, h], V[r, h], bias[:, h], t)
            w = weights(self_scores(q[r, h], K[r, h], bias[:, h], t))
            assert all(w[j] >= 0.25 for j in heavy[r]), (t, h, [float(w[j]) for j in heavy[r]])
            seen["last"] |= bites(ref[r, h], ref_self(q[r, h], K[r, h], V[r, h], bias[:, h], t, drop=[t]), vmax)
            if t >= ROUND:
                seen["second"] |= bites(ref[r, h], ref_self(q[r, h], K[r, h], V[r, h], bias[:, h], t, drop=[ROUND]), vmax)
            if t > 0:
                seen["bias"] |= bites(ref[r, h], ref_self(q[r, h], K[r, h], V[r, h], bias[:, h], t, shift=1), vmax)
            seen["head"] |= bites(ref[r, h], ref_self(q[r, h], K[r, h ^ 1], V[r, h ^ 1], bias[:, h ^ 1], t), vmax)
            seen["row"] |= bites(ref[r, h], ref_self(q[r, h], K[nb, h], V[nb, h], bias[:, h], t), vmax)
        assert all(seen.values()), ("the inputs of position %d cannot show this wrong kernel" % t, seen)
    ld, col0, W = 3 * H * 64, H * 64, H * 64
    B_ = be.buf(bias)
    got = np.zeros((rows, W), np.uint16)
    per = 38
    for r0 in range(0, rows, per):
        r1 = min(rows, r0 + per)
        n = r1 - r0
        ctx = new_ctx(be, n, ld)
        # pos_rows[row] + t_off is the position
        step_ex(be, bf(be, q[r0:r1]), bf(be, K[r0:r1]), bf(be, V[r0:r1]), ctx, n, H, 1, cap, bias=B_, t=-7, n_keys=-7, t_off=2,
                pos_rows=ibuf(be, np.array(SWEEP[r0:r1]) - 2), ctx_ld=ld, ctx_col0=col0)
        got[r0:r1] = read_ctx(ctx, n, W, ld, col0)
    assert_close(pk.bf16_to_f32(got).reshape(rows, H, 64), ref, vmax, "self form, pos_rows")
    for t in SAME_BITS:
        r = SWEEP.index(t)
        for how in ("host", "dev"):
            ctx = new_ctx(be, 1, ld)
            kw = dict(t=t, n_keys=t + 1) if how == "host" else dict(t=-7, n_keys=-7, t_dev=ibuf(be, [t - 5]), t_off=5)
            step_ex(be, bf(be, q[r:r + 1]), bf(be, K[r:r + 1]), bf(be, V[r:r + 1]), ctx, 1, H, 1, cap, bias=B_, ctx_ld=ld, ctx_col0=col0, **kw)
            assert np.array_equal(read_ctx(ctx, 1, W, ld, col0)[0], got[r]), (t, how)


# ---------------------------------------------------------------------------------------------------------------------------------
# b. beam self form (ancestor table: the 4-wave kernel)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("be_name", BACKENDS)
def test_beam_self_form_ancestor_table(be_name):
    """2 images x 5 beams, anc[j][row] random among the image's physical rows for every position j, positions 0 .. 511; the position
    is delivered by the host, through t_dev and through pos_rows in turn.  Rows share physical cache entries, so the heavy keys (the
    last one and key 128) are made through the bias table of the launch: distance 0 and distance t - 128 lifted."""
    be = get_backend(be_name)
    H, cap, nimg, G = 2, 512, 2, 5
    rows = nimg * G
    rs = np.random.RandomState(2002)
    q = pk.bf16_round(rs.standard_normal((rows, H, 64)) * 0.25)
    K = pk.bf16_round(rs.standard_normal((rows, H, cap, 64)) * 0.0625)       # scores std 0.125: the two lifted keys weigh about the same
    V = pk.bf16_round(rs.standard_normal((rows, H, cap, 64)) * 0.5)
    anc = np.zeros((cap, rows), np.int32)
    for j in range(cap):
        for r in range(rows):
            anc[j, r] = (r // G) * G + rs.randint(G)
    vmax = float(np.abs(V).max())
    Q, Kb, Vb, A = bf(be, q), bf(be, K), bf(be, V), be.buf(anc)
    ld, col0, W = 3 * H * 64, H * 64, H * 64
    jj = np.arange(cap)

    def gather(X, r, h, table):
        return X[table[:, r], h, jj]          # [cap][64]: position j lives in physical row table[j][r]

    for i, t in enumerate((0, 31, 32, 127, 128, 129, 300, 511)):
        bias = (rs.standard_normal((cap, H)) * 0.5).astype(np.float32)
        hv = [t] + ([ROUND] if t > ROUND else [])
        bias[[t - j for j in hv]] = np.float32(np.log(cap) + 6.0)
        ref = np.zeros((rows, H, 64))
        seen = dict(beam=False, image=False, head=False)
        anc_beam = anc.reshape(cap, nimg, G)[:, :, ::-1].reshape(cap, rows)      # another beam's history (same image)
        anc_img = anc.reshape(cap, nimg, G)[:, ::-1].reshape(cap, rows)           # the other image's rows
        for r in range(rows):
            row_seen = dict(last=False, second=t < ROUND, bias=t == 0)
            for h in range(H):
                Kr, Vr = gather(K, r, h, anc), gather(V, r, h, anc)
                ref[r, h] = ref_self(q[r, h], Kr, Vr, bias[:, h], t)
                w = weights(self_scores(q[r, h], Kr, bias[:, h], t))
                assert all(w[j] >= 0.25 for j in hv), (t, r, h, [float(w[j]) for j in hv])
                row_seen["last"] |= bites(ref[r, h], ref_self(q[r, h], Kr, Vr, bias[:, h], t, drop=[t]), vmax)
                if t >= ROUND:
                    row_seen["second"] |= bites(ref[r, h], ref_self(q[r, h], Kr, Vr, bias[:, h], t, drop=[ROUND]), vmax)
                if t > 0:
                    row_seen["bias"] |= bites(ref[r, h], ref_self(q[r, h], Kr, Vr, bias[:, h], t, shift=1), vmax)
                seen["beam"] |= bites(ref[r, h], ref_self(q[r, h], gather(K, r, h, anc_beam), gather(V, r, h, anc_beam), bias[:, h], t), vmax)
                seen["image"] |= bites(ref[r, h], ref_self(q[r, h], gather(K, r, h, anc_img), gather(V, r, h, anc_img), bias[:, h], t), vmax)
                seen["head"] |= bites(ref[r, h], ref_self(q[r, h], gather(K, r, h ^ 1, anc), gather(V, r, h ^ 1, anc), bias[:, h ^ 1], t), vmax)
            assert all(row_seen.values()), (t, r, row_seen)
        assert all(seen.values()), (t, seen)
        kw = [dict(t=t, n_keys=t + 1), dict(t=-7, n_keys=-7, t_dev=ibuf(be, [t + 3]), t_off=-3),
              dict(t=-7, n_keys=-7, pos_rows=ibuf(be, [t] * rows))][i % 3]
        ctx = new_ctx(be, rows, ld)
        step_ex(be, Q, Kb, Vb, ctx, rows, H, 1, cap, bias=be.buf(bias), anc=A, ctx_ld=ld, ctx_col0=col0, **kw)
        got = pk.bf16_to_f32(read_ctx(ctx, rows, W, ld, col0)).reshape(rows, H, 64)
        assert_close(got, ref, vmax, "beam self form, t = %d" % t)


# ---------------------------------------------------------------------------------------------------------------------------------
# c. cross form, every group size; d. window, dead rows; e. one workgroup per CU
# ---------------------------------------------------------------------------------------------------------------------------------
def cross_lens(be_name):
    lens = [1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257]
    cap = 320
    if be_name == "hip":
        lens += [1087, 1088, 1232]
        cap = 1280
    return lens + [cap], cap


def cross_inputs(lens, cap, G, H, seed, dup=(3, 10)):
    """owners with the given key counts; slots (images) read them through a non-identity kv_owner in which the slots `dup` share the
    owner of another slot; every row has its own deferred scale r in [0.6, 1.6].  Heavy keys per owner: the last and key 128."""
    rs = np.random.RandomState(seed)
    owners = len(lens)
    kvo = list(rs.permutation(owners))
    for i, d in enumerate(dup):
        kvo.insert(d, kvo[(d + 4 + i) % len(kvo)])
    kvo = np.array(kvo, np.int32)
    slots = len(kvo)
    rows = slots * G
    q = pk.bf16_round(rs.standard_normal((rows, H, 64)) * 0.5)
    q[:, :, 0] = 2.0
    K = pk.bf16_round(rs.standard_normal((owners, H, cap, 64)) * 0.5)
    V = pk.bf16_round(rs.standard_normal((owners, H, cap, 64)) * 0.5)
    nparts, inv_d, eps = 8, 1.0 / 8, 1e-6
    r_want = rs.uniform(0.6, 1.6, rows)
    part = (rs.uniform(0.5, 1.5, (rows, nparts)) / r_want[:, None] ** 2).astype(np.float32)
    r = row_scale(part, inv_d, eps)
    heavy = []
    for o, n in enumerate(lens):
        hv = sorted({n - 1} | ({ROUND} if n - 1 > ROUND else set()))
        heavy.append(hv)
        readers = [row for row in range(rows) if kvo[row // G] == o]
        for h in range(H):
            c = 2.0         # (for the reader that needs it most the rest keeps 20 %: a neighbour's scale then shows)
            for row in readers:
                s = cross_scores(q[row, h], K[o, h], n, r[row])
                c = max(c, (lse(np.delete(s, hv)) + np.log(4.0)) / (2.0 * r[row]))
            K[o, h, hv] = 0.0
            K[o, h, hv, 0] = bf16_exact_up(c)
    return q, K, V, kvo, part, r, (inv_d, eps), heavy


def cross_reference(q, K, V, lens, kvo, r, G, H, heavy, vmax, rows=None):
    """float64 reference [rows][H][64] after checking that the wrong kernels are visible"""
    rows = len(q) if rows is None else rows
    slots = len(kvo)
    ref = np.zeros((rows, H, 64))
    seen = dict(head=False, owner=False, scale=False)
    key_seen = {}
    for row in range(rows):
        o = kvo[row // G]
        n = lens[o]
        o2 = kvo[(row // G + 1) % slots]
        for h in range(H):
            ref[row, h] = ref_cross(q[row, h], K[o, h], V[o, h], n, r[row])
            w = weights(cross_scores(q[row, h], K[o, h], n, r[row]))
            assert all(w[j] >= 0.25 for j in heavy[o]), (row, h, n, [float(w[j]) for j in heavy[o]])
            for j in heavy[o]:
                key_seen[(row // G, j)] = key_seen.get((row // G, j), False) | bites(
                    ref[row, h], ref_cross(q[row, h], K[o, h], V[o, h], n, r[row], drop=[j]), vmax)
            seen["head"] |= bites(ref[row, h], ref_cross(q[row, h], K[o, h ^ 1], V[o, h ^ 1], n, r[row]), vmax)
            seen["owner"] |= bites(ref[row, h], ref_cross(q[row, h], K[o2, h], V[o2, h], lens[o2], r[row]), vmax)
            seen["scale"] |= bites(ref[row, h], ref_cross(q[row, h], K[o, h], V[o, h], n, r[(row + 1) % rows]), vmax)
    assert all(seen.values()) and all(key_seen.values()), (seen, [k for k, v in key_seen.items() if not v])
    return ref


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("G", [1, 2, 3, 4, 5, 6, 7, 8])
def test_cross_form_every_group(be_name, G):
    """Key counts 1 .. 257 around every 16 / 64 / 128 / 256 boundary (on the GPU also 1087, 1088, 1232) and the capacity; kv_owner
    non-identity with slots sharing an owner; per-row deferred scale given as partial sums; dead rows (G = 1) / a dead image slot
    (G > 1: all its rows flagged, as the beam queue does); context window in the middle third of the buffer."""
    be = get_backend(be_name)
    H = 2
    lens, cap = cross_lens(be_name)
    q, K, V, kvo, part, r, (inv_d, eps), heavy = cross_inputs(lens, cap, G, H, 3000 + G)
    rows, vmax = len(q), float(np.abs(V).max())
    ref = cross_reference(q, K, V, lens, kvo, r, G, H, heavy, vmax)
    dead_slots = [3, 10] if G == 1 else [3]         # slots 3 and 10 read an owner that another, live slot reads too
    live = np.ones(rows, np.int32)
    for s in dead_slots:
        live[s * G:(s + 1) * G] = 0
    dead = [int(x) for x in np.flatnonzero(live == 0)]
    ld, col0, W = 3 * H * 64, H * 64, H * 64
    ctx = new_ctx(be, rows, ld)
    step_ex(be, bf(be, q), bf(be, K), bf(be, V), ctx, rows, H, G, cap, lens=ibuf(be, lens), kv_owner=ibuf(be, kvo), live=ibuf(be, live),
            qrs=be.buf(part), inv_d=inv_d, eps=eps, ctx_ld=ld, ctx_col0=col0)
    got = pk.bf16_to_f32(read_ctx(ctx, rows, W, ld, col0, dead=dead)).reshape(rows, H, 64)
    alive = np.flatnonzero(live == 1)
    assert_close(got[alive], ref[alive], vmax, "cross form G = %d" % G)


@pytest.mark.parametrize("be_name", BACKENDS)
def test_cross_form_rows_not_a_multiple_of_the_group(be_name):
    """7 rows in groups of 5: the second owner has two rows, its three padded queries must not be written anywhere"""
    be = get_backend(be_name)
    H, G, cap, lens = 2, 5, 192, [129, 130]
    q, K, V, kvo, part, r, (inv_d, eps), heavy = cross_inputs(lens, cap, G, H, 3100, dup=())
    rows = 7
    q, part, r = q[:rows], part[:rows], r[:rows]
    vmax = float(np.abs(V).max())
    ref = cross_reference(q, K, V, lens, kvo, r, G, H, heavy, vmax, rows=rows)
    ld, col0, W = 3 * H * 64, H * 64, H * 64
    ctx = new_ctx(be, rows, ld)
    step_ex(be, bf(be, q), bf(be, K), bf(be, V), ctx, rows, H, G, cap, lens=ibuf(be, lens), kv_owner=ibuf(be, kvo), qrs=be.buf(part),
            inv_d=inv_d, eps=eps, ctx_ld=ld, ctx_col0=col0)
    assert_close(pk.bf16_to_f32(read_ctx(ctx, rows, W, ld, col0)).reshape(rows, H, 64), ref, vmax, "7 rows, G = 5")


@pytest.mark.gpu
def test_one_workgroup_per_cu_is_the_same_bits():
    """the residency cap of the in-flight runs (LDS request above half a CU) changes nothing that is computed: G = 1 cross, 32 rows"""
    be = get_backend("hip")
    H, cap, rows = 2, 1280, 32
    rs = np.random.RandomState(3200)
    lens = rs.randint(1000, cap + 1, rows).astype(np.int32)
    q, K, V = [bf(be, pk.bf16_round(rs.standard_normal(s) * 0.5)) for s in ((rows, H, 64), (rows, H, cap, 64), (rows, H, cap, 64))]
    outs = []
    for one in (0, 1, 0):
        ctx = new_ctx(be, rows, H * 64)
        step_ex(be, q, K, V, ctx, rows, H, 1, cap, lens=ibuf(be, lens), one_wg_per_cu=one)
        outs.append(read_ctx(ctx, rows, H * 64, H * 64, 0))
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
    assert not (outs[0] == SENT).all()


@pytest.mark.parametrize("be_name", BACKENDS)
def test_entries_reject_groups_without_a_kernel(be_name):
    be = get_backend(be_name)
    z = be.zeros((64,), np.uint16)
    for g in (0, 9, 16):
        assert be.lib.mgk_attention_step(be.stream, be.p(z), be.p(z), be.p(z), be.p(z), 1, 1, g, 64, None, 1, None, None, 0) == -1
    f = be.zeros((64,), np.float32)
    for g in (0, 5, 7, 9):
        assert step_rope(be, f, 64 * (g + 2), f, None, 0, 0, 1.0, z, z, z, 1, 1, g, 64) == -1, g


# ---------------------------------------------------------------------------------------------------------------------------------
# f. rotary grouped-query form
# ---------------------------------------------------------------------------------------------------------------------------------
def one_ulp(got, exact, ulps=1):
    """|got - exact| within one bf16 ulp of exact"""
    exact = np.asarray(exact, np.float64)
    e = np.floor(np.log2(np.maximum(np.abs(exact), 1e-30)))
    return bool((np.abs(np.asarray(got, np.float64) - exact) <= ulps * 2.0 ** (e - 7)).all())


def rope_inputs(positions, G, Hkv, cap, seed, with_rs):
    """pages = one sequence each (2 per position) + a spare page for the dead row.  Heavy keys: the new one (position t) and, in the
    cache, key 128: k = c*(cos t0, sin t0) on dims (0, 32), the direction all the group's rotated queries share (q[0] = 16 before the
    rotation), so both score alike."""
    rs = np.random.RandomState(seed)
    pages = 2 * len(positions) + 1
    pos_of_page = [positions[p // 2] for p in range(pages - 1)] + [positions[1]]
    width = (G + 2) * Hkv * 64
    ld = width + 64
    nparts, inv_d, eps = 8, 1.0 / 8, 1e-5
    cs = rope_table(cap)
    qscale = 0.125
    rows = pages
    owner = np.array(list(rs.permutation(pages - 1)), np.int32)
    dead_row = 4
    owner = np.insert(owner, dead_row, pages - 1).astype(np.int32)           # the dead row owns the spare page
    qkv = (rs.standard_normal((rows, ld))).astype(np.float32)
    part = (rs.uniform(0.5, 1.5, (rows, nparts)) / rs.uniform(0.7, 1.4, rows)[:, None] ** 2).astype(np.float32) if with_rs else None
    r = row_scale(part, inv_d, eps) if with_rs else np.ones(rows)
    Kc = pk.bf16_round(rs.standard_normal((pages, Hkv, cap, 64)) * 0.5)
    Vc = pk.bf16_round(rs.standard_normal((pages, Hkv, cap, 64)) * 0.5)
    Hq = G * Hkv
    c = 12.0
    for row in range(rows):
        p = int(owner[row])
        t = pos_of_page[p]
        for hq in range(Hq):
            qkv[row, hq * 64] = 16.0
        for h in range(Hkv):
            qkv[row, (Hq + h) * 64:(Hq + h + 1) * 64] *= 0.0625       # (little beside the heavy component: the new key scores like key 128)
            qkv[row, (Hq + h) * 64] = np.float32(c / r[row])               # the new key: c*(cos, sin) after scale and rotation
            if t > ROUND:
                Kc[p, h, ROUND] = 0.0
                Kc[p, h, ROUND, 0] = b16(c * np.float64(cs[t, 0]))
                Kc[p, h, ROUND, 32] = b16(c * np.float64(cs[t, 32]))
    return dict(pages=pages, rows=rows, pos_of_page=pos_of_page, ld=ld, cs=cs, qscale=qscale, owner=owner, dead_row=dead_row, qkv=qkv,
                part=part, r=r, inv_d=inv_d, eps=eps, Kc=Kc, Vc=Vc)


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("with_rs", [False, True])
@pytest.mark.parametrize("Hkv", [1, 3])
@pytest.mark.parametrize("G", [1, 2, 3, 4, 6, 8])
def test_rotary_form(be_name, G, Hkv, with_rs):
    """Positions 0, 1, 127, 128, 129 (GPU: also 4095 of 4224).  Queue delivery (pos_rows + t_off + t_off_rows[page], kv_owner, live,
    one dead row) against float64; batch delivery of the same sequences (host t / t_dev + t_off, no indirection): same bits in the
    context and in the caches.  Exactly one 64-element row per (live page, kv head) of each cache changes, at the page's position,
    within one bf16 ulp of the float64 rotation."""
    be = get_backend(be_name)
    positions = [0, 1, 127, 128, 129] + ([4095] if be_name == "hip" else [])
    cap = 4224 if be_name == "hip" else 192
    d = rope_inputs(positions, G, Hkv, cap, 5000 + 16 * G + 2 * Hkv + with_rs, with_rs)
    rows, pages, owner, cs, ld, qs = d["rows"], d["pages"], d["owner"], d["cs"], d["ld"], d["qscale"]
    Hq, W = G * Hkv, G * Hkv * 64
    vmax = float(max(np.abs(d["Vc"]).max(), np.abs(d["qkv"][:, (Hq + Hkv) * 64:(Hq + 2 * Hkv) * 64] * d["r"][:, None]).max()))
    ref = np.zeros((rows, Hq, 64))
    knew, vnew = np.zeros((rows, Hkv, 64)), np.zeros((rows, Hkv, 64))
    seen = dict(head=False, page=False)
    for row in range(rows):
        if row == d["dead_row"]:
            continue
        p = int(owner[row])
        t = d["pos_of_page"][p]
        p2 = int(owner[(row + 1) % rows]) if (row + 1) % rows != d["dead_row"] else int(owner[(row + 2) % rows])
        row_seen = dict(last=False, second=t <= ROUND, position=False)
        for h in range(Hkv):
            a = (d["qkv"][row], G, Hkv, h, t)
            o, knew[row, h], vnew[row, h] = ref_rope(*a, cs[t], d["r"][row], qs, d["Kc"][p, h], d["Vc"][p, h])
            ref[row, h * G:(h + 1) * G] = o
            qg, kx, _ = rope_new(d["qkv"][row], G, Hkv, h, cs[t], d["r"][row], qs)
            sc = np.concatenate([np.asarray(d["Kc"][p, h, :t], np.float64), pk.bf16_round(kx).astype(np.float64)[None]]) @ pk.bf16_round(qg[0])
            w = weights(sc)
            assert w[t] >= 0.25 and (t <= ROUND or w[ROUND] >= 0.25), (row, t, h, float(w[t]), float(w[min(t, ROUND)]))
            row_seen["last"] |= bites(o, ref_rope(*a, cs[t], d["r"][row], qs, d["Kc"][p, h], d["Vc"][p, h], drop=[t])[0], vmax)
            if t > ROUND:
                row_seen["second"] |= bites(o, ref_rope(*a, cs[t], d["r"][row], qs, d["Kc"][p, h], d["Vc"][p, h], drop=[ROUND])[0], vmax)
            # the rotation of the neighbouring position (the analogue of the bias read one distance off)
            # (q and the new k turn together, so below key 128 only the appended k row shows it: more than 4 ulp off)
            o1, k1, _ = ref_rope(*a, cs[t + 1], d["r"][row], qs, d["Kc"][p, h], d["Vc"][p, h])
            row_seen["position"] |= bites(o, o1, vmax) or not one_ulp(k1, knew[row, h], ulps=4)
            if Hkv > 1:
                h2 = (h + 1) % Hkv
                seen["head"] |= bites(o, ref_rope(d["qkv"][row], G, Hkv, h, t, cs[t], d["r"][row], qs, d["Kc"][p, h2], d["Vc"][p, h2])[0], vmax)
            seen["page"] |= bites(o, ref_rope(*a, cs[t], d["r"][row], qs, d["Kc"][p2, h], d["Vc"][p2, h])[0], vmax)
        assert all(row_seen.values()), (row, t, row_seen)
    assert seen["page"] and (seen["head"] or Hkv == 1), seen
    # queue delivery
    t_off = 3
    toff_pg = np.random.RandomState(7).randint(-2, 6, pages).astype(np.int32)
    pos_rows = np.array([d["pos_of_page"][int(owner[row])] - t_off - toff_pg[int(owner[row])] for row in range(rows)], np.int32)
    live = np.ones(rows, np.int32)
    live[d["dead_row"]] = 0
    ctx_ld, col0 = W + 128, 64
    ctx = new_ctx(be, rows, ctx_ld)
    QKV, CS, RS = be.buf(d["qkv"]), be.buf(cs), (be.buf(d["part"]) if with_rs else None)
    Kq, Vq = bf(be, d["Kc"]), bf(be, d["Vc"])
    assert step_rope(be, QKV, ld, CS, RS, d["inv_d"], d["eps"], qs, Kq, Vq, ctx, rows, Hkv, G, cap, t=-9, t_off=t_off, pos_rows=ibuf(be, pos_rows),
                     t_off_rows=ibuf(be, toff_pg), kv_owner=ibuf(be, owner), live=ibuf(be, live), ctx_ld=ctx_ld, ctx_col0=col0) == 0
    got_bits = read_ctx(ctx, rows, W, ctx_ld, col0, dead=[d["dead_row"]])
    alive = np.flatnonzero(live == 1)
    assert_close(pk.bf16_to_f32(got_bits).reshape(rows, Hq, 64)[alive], ref[alive], vmax, "rotary form, queue delivery")
    caches = {}
    for name, buf, before, new in (("K", Kq, d["Kc"], knew), ("V", Vq, d["Vc"], vnew)):
        after = np.array(buf.numpy(), copy=True).reshape(pages, Hkv, cap, 64)
        caches[name] = after
        changed = (after != pk.bf16_bits(before)).any(-1)                       # [pages][Hkv][cap]
        expect = np.zeros_like(changed)
        for row in alive:
            p = int(owner[row])
            expect[p, :, d["pos_of_page"][p]] = True
            assert one_ulp(pk.bf16_to_f32(after[p, :, d["pos_of_page"][p]]), new[row]), (name, row)
        assert np.array_equal(changed, expect), (name, "cache rows written", np.argwhere(changed != expect)[:6].tolist())
    # batch delivery: the two sequences of a position in a launch of their own
    row_of_page = {int(owner[row]): row for row in range(rows)}
    for i, t in enumerate(positions):
        pg = [2 * i, 2 * i + 1]
        rr = [row_of_page[p] for p in pg]
        Kb, Vb = bf(be, d["Kc"][pg]), bf(be, d["Vc"][pg])
        cb = new_ctx(be, 2, ctx_ld)
        kw = dict(t=t) if i % 2 == 0 else dict(t=-9, t_dev=ibuf(be, [t - 40]), t_off=40)
        assert step_rope(be, be.buf(d["qkv"][rr]), ld, CS, be.buf(d["part"][rr]) if with_rs else None, d["inv_d"], d["eps"], qs, Kb, Vb, cb, 2, Hkv, G,
                         cap, ctx_ld=ctx_ld, ctx_col0=col0, **kw) == 0
        assert np.array_equal(read_ctx(cb, 2, W, ctx_ld, col0), got_bits[rr]), ("context: batch delivery differs from the queue delivery", t)
        assert np.array_equal(np.asarray(Kb.numpy()).reshape(2, Hkv, cap, 64), caches["K"][pg]), t
        assert np.array_equal(np.asarray(Vb.numpy()).reshape(2, Hkv, cap, 64), caches["V"][pg]), t


# ---------------------------------------------------------------------------------------------------------------------------------
# g. score profiles that stress the online softmax
# ---------------------------------------------------------------------------------------------------------------------------------
N_PROF = 2 * ROUND + 37          # two full rounds and a masked tail round


def assert_spikes_bite(prof, names, ref_of, vmax):
    """dropping the key that stands 60 above the rest must be visible"""
    for i, name in enumerate(names):
        if name.startswith("spike_"):
            j = int(np.argmax(prof[name]))
            assert bites(ref_of(i, None), ref_of(i, [j]), vmax), name


@pytest.mark.parametrize("be_name", BACKENDS)
def test_score_profiles_self_form(be_name):
    """q = e_0 (head 0) / -e_0 (head 1: every profile mirrored), keys (s_j - bias) e_0 with a bias table of -4 / 0 / 4: the scores
    the kernel sees are exactly the profile (head 0) - unscaled T5 scores, tens and more.  The step kernel's own bound holds for every
    profile (emulator and float64 agree within it; no profile needed the wider fp32-online-softmax bound)."""
    be = get_backend(be_name)
    H, cap, n = 2, 512, N_PROF
    t = n - 1
    prof = profiles(n, ROUND)
    names = list(prof)
    rows = len(names)
    rs = np.random.RandomState(6001)
    bias = (4.0 * rs.randint(-1, 2, (cap, H))).astype(np.float32)          # -4, 0, 4: profile -+ bias stays exact in bf16
    q = np.zeros((rows, H, 64), np.float32)
    q[:, 0, 0], q[:, 1, 0] = 1.0, -1.0
    K = pk.bf16_round(rs.standard_normal((rows, H, cap, 64)) * 0.5)
    V = pk.bf16_round(rs.standard_normal((rows, H, cap, 64)) * 0.5)
    for i, name in enumerate(names):
        K[i, 0, :n, 0] = prof[name] - bias[t - np.arange(n), 0]
        K[i, 1, :n, 0] = prof[name] + bias[t - np.arange(n), 1]          # head 1 sees -profile
    assert np.array_equal(K, pk.bf16_round(K)), "profile scores are not exact in bf16"
    vmax = float(np.abs(V).max())
    ref = np.stack([[ref_self(q[i, h], K[i, h], V[i, h], bias[:, h], t) for h in range(H)] for i in range(rows)])
    assert_spikes_bite(prof, names, lambda i, drop: ref_self(q[i, 0], K[i, 0], V[i, 0], bias[:, 0], t, drop=drop), vmax)
    ctx = new_ctx(be, rows, H * 64)
    step_ex(be, bf(be, q), bf(be, K), bf(be, V), ctx, rows, H, 1, cap, bias=be.buf(bias), t=-7, n_keys=-7, pos_rows=ibuf(be, [t] * rows))
    got = pk.bf16_to_f32(read_ctx(ctx, rows, H * 64, H * 64, 0)).reshape(rows, H, 64)
    for i, name in enumerate(names):
        assert_close(got[i], ref[i], vmax, "self form, profile " + name)


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("G", [1, 3])
def test_score_profiles_cross_form(be_name, G):
    """one owner per profile, G rows each with q = g' e_0 for g' = 1, -1, 2 (mirrored and doubled profiles share the owner's stream)"""
    be = get_backend(be_name)
    H, cap, n = 2, 320, N_PROF
    prof = profiles(n, ROUND)
    names = list(prof)
    owners = len(names)
    rows = owners * G
    rs = np.random.RandomState(6002)
    q = np.zeros((rows, H, 64), np.float32)
    for row in range(rows):
        q[row, :, 0] = (1.0, -1.0, 2.0)[row % G]
    q[:, 1, 0] *= -1.0
    K = pk.bf16_round(rs.standard_normal((owners, H, cap, 64)) * 0.5)
    V = pk.bf16_round(rs.standard_normal((owners, H, cap, 64)) * 0.5)
    for i, name in enumerate(names):
        K[i, :, :n, 0] = prof[name]
    assert np.array_equal(K, pk.bf16_round(K))
    vmax = float(np.abs(V).max())
    ref = np.stack([[ref_cross(q[row, h], K[row // G, h], V[row // G, h], n) for h in range(H)] for row in range(rows)])
    assert_spikes_bite(prof, names, lambda i, drop: ref_cross(q[i * G, 0], K[i, 0], V[i, 0], n, drop=drop), vmax)
    ctx = new_ctx(be, rows, H * 64)
    step_ex(be, bf(be, q), bf(be, K), bf(be, V), ctx, rows, H, G, cap, lens=ibuf(be, [n] * owners))
    got = pk.bf16_to_f32(read_ctx(ctx, rows, H * 64, H * 64, 0)).reshape(rows, H, 64)
    for row in range(rows):
        assert_close(got[row], ref[row], vmax, "cross form G = %d, profile %s, row %d" % (G, names[row // G], row % G))


@pytest.mark.parametrize("be_name", BACKENDS)
def test_score_profiles_rotary_form(be_name):
    """G = 4 query heads on one key/value head.  The rotated query is a (cos t, sin t) on dims (0, 32); cached keys s_j (cos t, sin t) / a
    give the profile (up to the bf16 rounding of the two components, which the reference shares); the last score belongs to the new key."""
    be = get_backend(be_name)
    G, Hkv, cap, n = 4, 1, 320, N_PROF
    t = n - 1
    prof = profiles(n, ROUND)
    names = list(prof)
    rows = len(names)
    rs = np.random.RandomState(6003)
    cs = rope_table(cap)
    ld, qs = (G + 2) * 64, 0.125
    qkv = np.zeros((rows, ld), np.float32)
    sign = (1.0, -1.0, 0.5, 2.0)
    for g in range(G):
        qkv[:, g * 64] = 8.0 * sign[g]                     # rotated and scaled: sign * (cos t, sin t)
    qkv[:, (G + 1) * 64:] = rs.standard_normal((rows, 64)) * 0.5
    Kc = np.zeros((rows, Hkv, cap, 64), np.float32)
    Vc = pk.bf16_round(rs.standard_normal((rows, Hkv, cap, 64)) * 0.5)
    c0, s0 = np.float64(cs[t, 0]), np.float64(cs[t, 32])
    for i, name in enumerate(names):
        Kc[i, 0, :t, 0] = pk.bf16_round((prof[name][:t] * c0).astype(np.float32))
        Kc[i, 0, :t, 32] = pk.bf16_round((prof[name][:t] * s0).astype(np.float32))
        qkv[i, G * 64] = np.float32(prof[name][t])
    vmax = float(max(np.abs(Vc).max(), np.abs(qkv[:, (G + 1) * 64:]).max()))
    ref = np.stack([ref_rope(qkv[i], G, Hkv, 0, t, cs[t], 1.0, qs, Kc[i, 0], Vc[i, 0])[0] for i in range(rows)])
    assert_spikes_bite(prof, names, lambda i, drop: ref_rope(qkv[i], G, Hkv, 0, t, cs[t], 1.0, qs, Kc[i, 0], Vc[i, 0], drop=drop)[0][0], vmax)
    ctx = new_ctx(be, rows, G * 64)
    assert step_rope(be, be.buf(qkv), ld, be.buf(cs), None, 0.0, 0.0, qs, bf(be, Kc), bf(be, Vc), ctx, rows, Hkv, G, cap, t=t) == 0
    got = pk.bf16_to_f32(read_ctx(ctx, rows, G * 64, G * 64, 0)).reshape(rows, G, 64)
    for i, name in enumerate(names):
        assert_close(got[i], ref[i], vmax, "rotary form, profile " + name)


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("n", [53, 165])
def test_score_profiles_absorbed_stream(be_name, n):
    """mgk_xattn and mgk_xattn_beams (rings of 3 and 4 stages, 1 - 3 key splits; 53 keys = 4 stages, of which three splits take 2 + 2 + 0)
    on the profiles in units of the stream's 16-key stages.  Wk_h[0] = e_0 and q = +-e_0 make the score of key j exactly +-enc[j][0];
    Wv has no weight on that feature, so V stays of order 1.  Bound: the rule of test_absorbed_cross_attention - the error against float64
    at most twice what the K / V form's own roundings (K, V, P, ctx in bf16) cost on the same inputs, plus its epsilon."""
    be = get_backend(be_name)
    d, H, cap, G = 128, 2, 176, 2
    inner = H * 64
    prof = profiles(n, 16)
    names = list(prof)
    owners = len(names)
    rows = owners * G
    rs = np.random.RandomState(6004)
    wkv = pk.bf16_round(rs.standard_normal((2 * inner, d)) / np.sqrt(d))
    for h in range(H):
        wkv[h * 64] = 0.0
        wkv[h * 64, 0] = 1.0
    wkv[inner:, 0] = 0.0
    enc = pk.bf16_round(rs.standard_normal((owners, cap, d)))
    enc[:, n:] = 0.0                                        # (the stream reads whole stages: the rows behind the last key are kept zero)
    for i, name in enumerate(names):
        enc[i, :n, 0] = prof[name]
    assert np.array_equal(enc, pk.bf16_round(enc))
    q = np.zeros((rows, H, 64), np.float32)
    q[0::2, 0, 0], q[0::2, 1, 0], q[1::2, 0, 0], q[1::2, 1, 0] = 1.0, -1.0, -1.0, 1.0
    ref, kvf = np.zeros((rows, H, 64)), np.zeros((rows, H, 64))
    for row in range(rows):
        e = enc[row // G, :n].astype(np.float64)
        for h in range(H):
            Kx, Vx = e @ wkv[h * 64:(h + 1) * 64].T.astype(np.float64), e @ wkv[inner + h * 64:inner + (h + 1) * 64].T.astype(np.float64)
            s = Kx @ q[row, h]
            ref[row, h] = attend(s, Vx)
            Kb, Vb = pk.bf16_round(Kx).astype(np.float64), pk.bf16_round(Vx).astype(np.float64)
            kvf[row, h] = pk.bf16_round(pk.bf16_round(weights(Kb @ q[row, h])).astype(np.float64) @ Vb)
    for i, name in enumerate(names):
        if name.startswith("spike_"):
            j = int(np.argmax(prof[name]))
            e = enc[i, :n].astype(np.float64)
            Vx = e @ wkv[inner:inner + 64].T.astype(np.float64)
            assert np.abs(attend(e[:, 0], Vx, drop=[j]) - ref[i * G, 0]).max() > 4 * (2.0 * np.abs(kvf - ref).max() + 2e-3), name
    e_kv = np.abs(kvf - ref)
    Q, Wb, E = bf(be, q), be.buf(wkv), bf(be, enc)
    L, KVR = ibuf(be, [n] * owners), ibuf(be, np.repeat(np.arange(owners), G))
    for nstg in (3, 4):
        for nsplit in (1, 2, 3):
            for beams in (False, True):
                ctx = be.zeros((((rows + 31) // 32 * 32) * inner,), np.uint16)
                wk, wv = be.zeros((H * d * 64,), np.uint16), be.zeros((H * d * 64,), np.uint16)
                qx = be.zeros((rows * H * d,), np.uint16)
                part, ml = be.zeros((rows * nsplit * H * d,), np.uint16), be.zeros((rows * nsplit * H * 2,), np.float32)
                if beams:
                    rc = be.lib.mgk_xattn_beams(be.stream, be.p(Q), be.p(Wb), be.p(E), be.p(L), None, None, rows, H, d, cap, G, nsplit, nstg, 0, 1,
                                                be.p(wk), be.p(wv), be.p(qx), be.p(part), be.p(ml), be.p(ctx))
                else:
                    rc = be.lib.mgk_xattn(be.stream, be.p(Q), be.p(Wb), be.p(E), be.p(L), be.p(KVR), rows, H, d, cap, nsplit, nstg,
                                          be.p(wk), be.p(wv), be.p(qx), be.p(part), be.p(ml), be.p(ctx))
                assert rc == 0, rc
                got = pk.unpack_tiles(ctx.numpy(), rows, inner).reshape(rows, H, 64)
                e_abs = np.abs(got - ref)
                what = (nstg, nsplit, "beams" if beams else "rows")
                assert np.isfinite(got).all(), what
                for i, name in enumerate(names):
                    ea, ek = e_abs[i * G:(i + 1) * G], e_kv[i * G:(i + 1) * G]
                    assert ea.max() <= 2.0 * ek.max() + 2e-3 and ea.mean() <= 2.0 * ek.mean() + 2e-4, (what, name, float(ea.max()), float(ek.max()),
                                                                                                   float(ea.mean()), float(ek.mean()))
