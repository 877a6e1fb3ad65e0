"""On-device sampling, kernel level: sample_select_kernel (csrc/k_sample.hip) through mgk_sample_select, its generator through mgk_philox.

The reference is written here from the rules of include/mgrapher.h (mg_sample_opts), in float64: MinLength, temperature, top-k with ties,
top-p with the boundary ties kept, inverse CDF in token-index order at u = r / 2^64, r from a pure-Python Philox4x32-10.

The allowance eps.  The kernel works on fixed-point masses m_i = rint(expf(q_i) * 2^32), q_i = (x_i - max) / T in float32, clamped to
2^32 - 1.  Against the float64 exp(q_i) of the exact quotient:
  - q_i carries two float32 roundings (the difference, the quotient): |dq| <= |q| * 2^-23, and only q >= -22.9 gives a non-zero mass,
    so exp(q) moves by at most 23 * 2^-23 relative;
  - expf is within 2 ulp in both builds (glibc < 1 ulp, the device library's documented bound is 1 ulp): 2^-22 relative;
  - rint and the clamp move a mass by at most one unit of 2^-32.
With rho = 23 * 2^-23 + 2^-22, every cumulative mass c and the total Z = sum exp(q) >= 1 (the maximum has exp(0) = 1 and always survives)
are known to the kernel within rho * c + V * 2^-32, so a normalised CDF edge c / Z moves by at most EPS = 2 * rho + 2 * V * 2^-32 (the
floor of __umul64hi is one more unit, inside the second term's slack since fewer than V tokens precede any edge).  The same EPS bounds
the top-p comparison "ascending mass / Z > 1 - top_p".  A draw whose u lies within EPS of an edge of its interval may land on the
neighbour; a row whose top-p boundary lies within EPS may keep or drop the boundary value's tokens.  Top-k compares floats: no allowance.
Each case asserts that at most 1 % of its draws need the allowance - by the float64 reference alone and for the kernel's answers."""
import ctypes as C
import math

import numpy as np
import pytest

from tests.backends import get_backend

BACKENDS = [pytest.param("emu"), pytest.param("hip", marks=pytest.mark.gpu)]
RHO = 23 * 2.0 ** -23 + 2.0 ** -22
M32 = 0xFFFFFFFF


def eps_of(V):
    return 2 * RHO + 2 * V * 2.0 ** -32


# ---- Philox4x32-10 from its definition (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) ----
def philox4x32_10(seed, stream, pos):
    c = [stream & M32, (stream >> 32) & M32, pos & M32, 0]
    k = [seed & M32, (seed >> 32) & M32]
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & M32, (p0 >> 32) ^ c[3] ^ k[1], p0 & M32]
        k = [(k[0] + 0x9E3779B9) & M32, (k[1] + 0xBB67AE85) & M32]
    return c


def draw_u(seed, stream, pos):
    w = philox4x32_10(seed, stream, pos)
    return ((w[1] << 32) | w[0]) / 2.0 ** 64


def _declare(lib):
    lib.mgk_sample_select.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int,
                                      C.c_float, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_int]
    lib.mgk_philox.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint32)]


def padded(lg):
    rows, V = lg.shape
    ldl = (V + 31) // 32 * 32
    out = np.full((rows, ldl), 7.0e37, np.float32)       # the padding must never be read as a logit: it would win every row
    out[:, :V] = lg
    return out, ldl


def run_sample(be, lg, eos, pad, min_len, T, top_k, top_p, seed, pos, sids=None, unf=None, max_len=8, scores=True):
    _declare(be.lib)
    rows, V = lg.shape
    L, ldl = padded(lg)
    unf = np.ones(rows, np.int32) if unf is None else unf.astype(np.int32)
    nxt, out = be.zeros((rows,), np.int64), be.buf(np.full((rows, max_len), -7, np.int64))
    ub, nu = be.buf(unf), be.zeros((1,), np.int32)
    ts = be.buf(np.full((rows, max_len - 1), 9.0, np.float32)) if scores else None
    sb = be.buf(np.asarray(sids, np.uint64).view(np.int64)) if sids is not None else None
    rc = be.lib.mgk_sample_select(be.stream, be.p(be.buf(L)), rows, V, ldl, eos, pad, min_len, T, top_k, top_p, seed, be.p(sb), be.p(nxt),
                                  be.p(out), max_len, pos, be.p(ub), be.p(nu), be.p(ts), max_len - 1)
    assert rc == 0
    return dict(next=nxt.numpy().copy(), out=out.numpy().copy(), unf=ub.numpy().copy(), n_unf=int(nu.numpy()[0]),
                ts=ts.numpy().copy() if scores else None)


# ---- the float64 reference ----
class RefRow:
    """Survivors and CDF of one row by the rules; `alt` = the survivor set with the top-p boundary value decided the other way, when
    the boundary lies within eps."""

    def __init__(self, x32, suppressed, T, top_k, top_p, eps):
        x = x32.astype(np.float64)
        alive = np.ones(x.shape, bool)
        if suppressed is not None:
            alive[suppressed] = False
        keep = alive.copy()
        if top_k > 0:
            k = min(top_k, int(alive.sum()))
            kth = np.sort(x32[alive])[-k]
            keep &= x32 >= kth
        e = np.where(alive, np.exp((x - x[alive].max()) / T), 0.0)
        self.e = e
        self.alt = None
        if top_p < 1.0:
            idx = np.flatnonzero(keep)
            order = idx[np.argsort(x32[idx], kind="stable")]
            vals = x32[order]
            cum = np.cumsum(e[order])
            total = cum[-1]
            last = np.r_[vals[1:] != vals[:-1], True]                 # last element of every run of equal values
            run_end = np.flatnonzero(last)
            asc = cum[run_end]                                        # ascending mass up to and including each distinct value
            run_of = np.cumsum(np.r_[False, last[:-1]])               # run index of every element
            frac = asc / total
            kept_run = frac > 1.0 - top_p
            kept_run[-1] = True                                       # at least the maximum
            near = np.flatnonzero(np.abs(frac - (1.0 - top_p)) <= eps)
            new = np.zeros(x.shape, bool)
            new[order] = kept_run[run_of]
            if len(near):
                alt_run = kept_run.copy()
                alt_run[near] = ~alt_run[near]
                alt_run[-1] = True
                self.alt = np.zeros(x.shape, bool)
                self.alt[order] = alt_run[run_of]
            keep = new
        self.keep = keep

    def cdf(self, keep):
        c = np.cumsum(np.where(keep, self.e, 0.0))
        return c / c[-1]

    def judge(self, tok, u, eps):
        """-> 'exact' | 'eps' | None for the kernel's token."""
        for n, keep in enumerate([self.keep] + ([self.alt] if self.alt is not None else [])):
            if not keep[tok]:
                continue
            c = self.cdf(keep)
            lo, hi = (c[tok - 1] if tok else 0.0), c[tok]
            if n == 0 and lo <= u < hi:
                return "exact"
            if lo - eps <= u < hi + eps:
                return "eps"
        return None

    def needs_allowance(self, u, eps):
        """By the reference alone: u within eps of an edge of its own interval, or the top-p boundary within eps."""
        if self.alt is not None:
            return True
        c = self.cdf(self.keep)
        t = int(np.searchsorted(c, u, side="right"))
        lo, hi = (c[t - 1] if t else 0.0), c[min(t, len(c) - 1)]
        return u - lo < eps or hi - u <= eps

    def logp(self, tok):
        return math.log(self.e[tok] / np.where(self.keep, self.e, 0.0).sum())


def logits_for(rows, V, seed, sigma):
    return (np.random.default_rng(seed).standard_normal((rows, V)) * sigma).astype(np.float32)


@pytest.mark.parametrize("be_name", BACKENDS)
def test_philox_matches_definition(be_name):
    be = get_backend(be_name)
    _declare(be.lib)
    rng = np.random.default_rng(5)
    out = (C.c_uint32 * 4)()
    triples = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (2 ** 64 - 1, 2 ** 64 - 1, 2 ** 32 - 1)]
    triples += [(int(rng.integers(0, 2 ** 63)) * 2 + 1, int(rng.integers(0, 2 ** 63)), int(rng.integers(0, 2 ** 31))) for _ in range(300)]
    for seed, stream, pos in triples:
        assert be.lib.mgk_philox(seed, stream, pos, out) == 0
        assert list(out) == philox4x32_10(seed, stream, pos), (seed, stream, pos)


# (T, top_k, top_p): each filter alone, pairs, all three, the clamp of k
# (a top-p boundary is decided within EPS only where the boundary token's own probability is well above 200 * EPS = 0.1 - 0.4 %: top_p
# close to 1 cuts among tokens smaller than that, so the grid's top_p values cut among the large ones)
GRID = [(1.0, 0, 1.0), (0.7, 0, 1.0), (1.0, 50, 1.0), (1.0, 0, 0.9), (0.8, 20, 0.95), (1.3, 5, 0.5), (1.0, 10 ** 6, 0.7)]
# sigma: the logits' spread.  The large vocabulary needs a peaked row for the unfiltered cases: EPS is 2e-5 there, and a flat row of
# 33 201 tokens has intervals of that width (a model's logits at a decode step are peaked, too)
SHAPES = [pytest.param(500, 128, 5.0, id="V500"), pytest.param(33201, 128, 9.0, id="V33201"),
          pytest.param(33201, 256, 9.0, id="V33201-256rows")]


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("V,rows,sigma", SHAPES)
def test_exact_rule_parity(be_name, V, rows, sigma):
    be = get_backend(be_name)
    eos, pad, eps = 1, 0, eps_of(V)
    grid = GRID if rows < 256 else GRID[4:5]
    for gi, (T, k, p) in enumerate(grid):              # a case = one (V, T, top_k, top_p) over its positions
        n_eps = n_ref = n_draws = 0
        for pos, min_len in ((1, 0), (3, 6)) if rows < 256 else ((2, 0),):      # EOS live / suppressed by MinLength
            lg = logits_for(rows, V, 100 + gi, sigma)
            lg[::3, eos] = lg[::3].max(-1) + 1.0                                # EOS is the favourite of a third of the rows
            seed = 0x1234ABCD5678 + gi
            sids = np.arange(rows, dtype=np.uint64) * 977 + 5
            r = run_sample(be, lg, eos, pad, min_len, T, k, p, seed, pos, sids=sids)
            n_draws += rows
            for b in range(rows):
                ref = RefRow(lg[b], eos if pos < min_len else None, T, k, p, eps)
                u = draw_u(seed, int(sids[b]), pos)
                tok = int(r["next"][b])
                verdict = ref.judge(tok, u, eps)
                assert verdict is not None, (T, k, p, pos, b, tok, u)
                n_eps += verdict == "eps"
                n_ref += ref.needs_allowance(u, eps)
                assert r["out"][b, pos] == tok
                assert r["unf"][b] == (tok != eos)
                assert abs(r["ts"][b, pos - 1] - ref.logp(tok)) < 1e-4 or verdict == "eps"
            assert r["n_unf"] == int(r["unf"].sum())
        print(f"V={V} rows={rows} T={T} k={k} p={p}: allowance used {n_eps}/{n_draws}, by the reference alone {n_ref}/{n_draws}")
        assert n_ref <= 0.01 * n_draws, "the case's inputs lean on the allowance"
        assert n_eps <= 0.01 * n_draws


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("V", [500, 33201])
def test_degenerate_cases_equal_greedy(be_name, V):
    """top_k = 1, and a top_p that keeps one token: ids, unfinished and n_unfinished bit-equal to mgk_greedy_select, finished rows included."""
    be = get_backend(be_name)
    rows, eos, pad, max_len = 48, 1, 0, 8
    lg = logits_for(rows, V, 7, 2.0)
    lg[::4, eos] = lg[::4].max(-1) + 0.5
    srt = np.sort(lg, -1)
    assert np.all(srt[:, -1] > srt[:, -2]), "exact top-1 tie in the inputs"
    unf0 = np.ones(rows, np.int32)
    unf0[[3, 17]] = 0
    L, ldl = padded(lg)
    for pos, min_len in ((2, 0), (2, 5)):
        if pos < min_len:
            m = lg.copy()
            m[:, eos] = -np.inf
            s2 = np.sort(m, -1)
            assert np.all(s2[:, -1] > s2[:, -2])
        nxt, out = be.zeros((rows,), np.int64), be.buf(np.full((rows, max_len), -7, np.int64))
        ub, nu = be.buf(unf0), be.zeros((1,), np.int32)
        assert be.lib.mgk_greedy_select(be.stream, be.p(be.buf(L)), rows, V, ldl, eos, pad, min_len, be.p(nxt), be.p(out), max_len, pos,
                                        be.p(ub), be.p(nu), None) == 0
        g = dict(next=nxt.numpy().copy(), out=out.numpy().copy(), unf=ub.numpy().copy(), n_unf=int(nu.numpy()[0]))
        for T, k, p in ((1.0, 1, 1.0), (0.6, 1, 0.9), (1.0, 0, 1e-6), (1.0, 40, 1e-6)):
            r = run_sample(be, lg, eos, pad, min_len, T, k, p, 99, pos, unf=unf0, max_len=max_len)
            assert np.array_equal(r["next"], g["next"]) and np.array_equal(r["out"], g["out"])
            assert np.array_equal(r["unf"], g["unf"]) and r["n_unf"] == g["n_unf"]
            assert np.all(r["next"][[3, 17]] == pad)
            assert np.all(r["ts"][:, pos - 1] == 0.0), "one survivor: log-probability 0"
            assert np.all(np.delete(r["ts"], pos - 1, axis=1) == 9.0), "only the step's column is written"


def chi2_quantile(df, z):
    """Wilson-Hilferty: the chi-square quantile at the normal deviate z."""
    return df * (1 - 2 / (9 * df) + z * math.sqrt(2 / (9 * df))) ** 3


@pytest.mark.parametrize("be_name", BACKENDS)
@pytest.mark.parametrize("top_k", [0, 8])
def test_distribution_chi_square(be_name, top_k):
    """One row of 64 logits, 256 rows x 800 positions = 204 800 draws at a fixed seed: chi-square against the softmax (top_k = 8: the
    renormalised top 8) below the 1 - 1e-6 quantile.  Deterministic: the draws are a pure function of (seed, row, position)."""
    be = get_backend(be_name)
    V, rows, npos = 64, 256, 800
    x = (np.random.default_rng(3).standard_normal(V) * 1.5).astype(np.float32)
    lg = np.tile(x, (rows, 1))
    counts = np.zeros(V, np.int64)
    for pos in range(1, npos + 1):
        r = run_sample(be, lg, -1, 0, 0, 1.0, top_k, 1.0, 20240607, pos, max_len=npos + 1, scores=False)
        counts += np.bincount(r["next"], minlength=V)
    n = rows * npos
    assert counts.sum() == n >= 200000
    e = np.exp(x.astype(np.float64) - x.max())
    if top_k:
        e[x < np.sort(x)[-top_k]] = 0.0
    pr = e / e.sum()
    assert np.all(counts[pr == 0] == 0)
    live = pr > 0
    assert np.all(n * pr[live] > 5), "expected counts too small for the chi-square approximation"
    stat = float((((counts - n * pr) ** 2)[live] / (n * pr[live])).sum())
    df = int(live.sum()) - 1
    bound = chi2_quantile(df, 4.753424)                  # normal deviate of 1 - 1e-6
    print(f"chi-square {stat:.1f} at {df} degrees of freedom, bound {bound:.1f}")
    assert stat < bound


@pytest.mark.parametrize("be_name", BACKENDS)
def test_token_scores_are_warped_log_probabilities(be_name):
    be = get_backend(be_name)
    V, rows, eos = 500, 96, 1
    for gi, (T, k, p, pos, min_len) in enumerate([(1.0, 0, 1.0, 1, 0), (0.7, 0, 1.0, 2, 4), (1.0, 30, 1.0, 1, 0), (1.2, 0, 0.8, 3, 0),
                                                  (0.9, 25, 0.9, 2, 6)]):
        lg = logits_for(rows, V, 40 + gi, 2.5)
        r = run_sample(be, lg, eos, 0, min_len, T, k, p, 777 + gi, pos)
        worst = 0.0
        for b in range(rows):
            ref = RefRow(lg[b], eos if pos < min_len else None, T, k, p, eps_of(V))
            tok = int(r["next"][b])
            if ref.alt is not None and not ref.keep[tok]:
                continue                                  # the top-p boundary itself is within eps: the normaliser is the other set's
            assert ref.keep[tok]
            if ref.alt is None:
                worst = max(worst, abs(r["ts"][b, pos - 1] - ref.logp(tok)))
        print(f"T={T} k={k} p={p}: max |token score - float64 log p| = {worst:.2e}")
        assert worst < 1e-4


@pytest.mark.parametrize("be_name", BACKENDS)
def test_determinism_seed_and_stream_ids(be_name):
    be = get_backend(be_name)
    V, rows = 500, 64
    lg = logits_for(rows, V, 9, 1.5)
    sids = (np.arange(rows, dtype=np.uint64) + 1) * 1000003
    a = run_sample(be, lg, 1, 0, 0, 0.9, 40, 0.95, 11, 2, sids=sids)
    b = run_sample(be, lg, 1, 0, 0, 0.9, 40, 0.95, 11, 2, sids=sids)
    for key in ("next", "out", "unf", "ts"):
        assert np.array_equal(a[key], b[key])
    c = run_sample(be, lg, 1, 0, 0, 0.9, 40, 0.95, 12, 2, sids=sids)
    assert not np.array_equal(a["next"], c["next"])
    d = run_sample(be, lg, 1, 0, 0, 0.9, 40, 0.95, 11, 3, sids=sids)
    assert not np.array_equal(a["next"], d["next"]), "the position is part of the counter"
    perm = np.random.default_rng(1).permutation(rows)
    e = run_sample(be, lg[perm], 1, 0, 0, 0.9, 40, 0.95, 11, 2, sids=sids[perm])
    assert np.array_equal(e["next"], a["next"][perm]) and np.array_equal(e["ts"], a["ts"][perm])
    # default stream ids = the row index
    f = run_sample(be, lg, 1, 0, 0, 0.9, 40, 0.95, 11, 2)
    g = run_sample(be, lg, 1, 0, 0, 0.9, 40, 0.95, 11, 2, sids=np.arange(rows, dtype=np.uint64))
    assert np.array_equal(f["next"], g["next"])


@pytest.mark.parametrize("be_name", BACKENDS)
def test_argument_errors(be_name):
    be = get_backend(be_name)
    _declare(be.lib)
    lg = logits_for(4, 64, 1, 1.0)
    L, ldl = padded(lg)
    args = lambda T, k, p, V=64: (be.stream, be.p(be.buf(L)), 4, V, ldl, 1, 0, 0, T, k, p, 1, None, be.p(be.zeros((4,), np.int64)),
                                  be.p(be.zeros((4, 8), np.int64)), 8, 1, be.p(be.buf(np.ones(4, np.int32))), be.p(be.zeros((1,), np.int32)),
                                  None, 7)
    assert be.lib.mgk_sample_select(*args(0.0, 0, 1.0)) < 0
    assert be.lib.mgk_sample_select(*args(-1.0, 0, 1.0)) < 0
    assert be.lib.mgk_sample_select(*args(1.0, -1, 1.0)) < 0
    assert be.lib.mgk_sample_select(*args(1.0, 0, 1.0)) == 0
