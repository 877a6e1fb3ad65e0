"""Scripted logits for beam search, and a plain float64 restatement of stock transformers 5.15 `_beam_search`
(generation/utils.py:3208-3525) to check the device beam step (k_beam.hip) and the oracle against.

A script is a pure function `logits(image, prefix) -> float32[V]` (prefix = the start token and the tokens chosen so far).
Each row is a constant base value with a few dozen "hot" tokens, seeded by a CRC of (seed, image, prefix), so a 512-step
run over 160 rows stays cheap on the host and every machine draws the same rows.  Two kinds:

  soft  hot values uniform in [-40, 0), base -20: every column contributes to the log-sum-exp.  Near-ties can happen by
        chance; the reference refuses them (below), so a case that uses soft rows takes the first seed without one
        (`tie_free`).
  grid  top token 0, the other hot tokens at -41, -42, ... and base -80: the log-sum-exp is exactly 0 in float32 and float64,
        so every log-probability and running score is an integer and every comparison is an exact tie or at least 1 apart
        (the length-penalty division aside).  Long runs use these.

The reference selects by the explicit rule: value descending, then flat index ascending.  At every selection it looks at
the neighbours up to the first dropped candidate: they must be tied (|difference| <= 1e-9, float64 rounding of equal
sums) or at least 1e-3 apart; otherwise it raises NearTie, so a scenario cannot flake between float32 and float64.
Values gated with -1e9 (stock's masks) are not checked: float32 rounds them onto a 64-wide grid, and which of them fill
the unfinished slots of the finished set never reaches an output.
"""
import math
import zlib

import numpy as np

TIE = 1e-9
MARGIN = 1e-3
GATED = -5.0e8


class NearTie(AssertionError):
    pass


class Script:
    def __init__(self, V, eos, seed=0, kind="soft", n_hot=24, eos_rank=None, same_rows=False, dup=0, big=None, uniform_every=0):
        """eos_rank(image, cur_len) -> None (EOS stays a base token) or r >= 1 (EOS takes the row's r-th best hot value);
        same_rows: a row depends on (image, step) only, so beams with equal running scores tie across rows;
        dup: that many hot tokens repeat the value of another one below the top (ties inside a row);
        big: +-1e4 added to the rows of odd / even (image + step) (big = 1e4);
        uniform_every: every row of a step with cur_len % uniform_every == 0 is uniform."""
        assert kind in ("soft", "grid") and V > n_hot + 2
        self.V, self.eos, self.seed, self.kind, self.n_hot = V, eos, seed, kind, n_hot
        self.eos_rank, self.same_rows, self.dup, self.big, self.uniform_every = eos_rank, same_rows, dup, big, uniform_every
        self.base = np.float32(-20.0 if kind == "soft" else -80.0)

    def row(self, image, prefix):
        """(hot tokens int64 [n], hot values float32 [n], base value float32); tokens distinct."""
        cur_len = len(prefix)
        if self.uniform_every and cur_len % self.uniform_every == 0:
            return np.zeros(0, np.int64), np.zeros(0, np.float32), np.float32(-1.5)
        key = (self.seed, image, cur_len) if self.same_rows else (self.seed, image, tuple(int(t) for t in prefix))
        rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
        n = self.n_hot
        toks = []
        for t in rng.integers(0, self.V, 4 * n):
            if t != self.eos and t not in toks:
                toks.append(int(t))
                if len(toks) == n:
                    break
        if self.kind == "soft":
            vals = -rng.uniform(0.0, 40.0, n)
        else:
            vals = np.concatenate([[0.0], -(41.0 + rng.permutation(n - 1))])
        for i in range(2, min(self.dup + 1, n - 1) + 1):     # (never the top value: grid rows keep a log-sum-exp of 0)
            vals[i] = vals[rng.integers(1, i)]
        vals = np.sort(vals)[::-1].astype(np.float32)
        toks = np.array(toks, np.int64)
        r = self.eos_rank(image, cur_len) if self.eos_rank else None
        if r is not None and 1 <= r <= n:
            toks[r - 1] = self.eos
        base = self.base
        if self.big is not None:
            off = np.float32(self.big if (image + cur_len) % 2 else -self.big)
            vals = (vals + off).astype(np.float32)
            base = np.float32(base + off)
        return toks, vals, base

    def logits(self, image, prefix):
        toks, vals, base = self.row(image, prefix)
        out = np.full(self.V, base, np.float32)
        out[toks] = vals
        return out

    def log_probs(self, image, prefix, no_eos):
        """float64 processed log-probabilities of a sparse candidate set that holds the row's best 2*8+2 tokens in the selection
        order: (tokens, lp).  lse by an exactly rounded sum over the row's multiset of values."""
        toks, vals, base = self.row(image, prefix)
        v = vals.astype(np.float64)
        n_base = self.V - len(toks)
        b = float(base)
        mx = max(v.max() if len(v) else -np.inf, b if n_base else -np.inf)
        lse = math.log(math.fsum([math.exp(x - mx) for x in v] + [n_base * math.exp(b - mx)]))
        hot = set(toks.tolist())
        extra = []
        t = 0
        while len(extra) < 18 and t < self.V:
            if t not in hot:
                extra.append(t)
            t += 1
        all_t = np.concatenate([toks, np.array(extra, np.int64)])
        all_v = np.concatenate([v, np.full(len(extra), b)])
        lp = (all_v - mx) - lse
        if no_eos:
            lp[all_t == self.eos] = -np.inf
        return all_t, lp


def tie_free(make, run, seeds=range(64)):
    """(script, result) for the first seed whose reference run raises no NearTie: make(seed) -> Script, run(script) -> result."""
    for seed in seeds:
        script = make(seed)
        try:
            return script, run(script)
        except NearTie:
            continue
    raise AssertionError("no seed without a near-tie")


def select(values, index, n):
    """positions of the first n of `values` by (value descending, index ascending), values within TIE counted equal;
    raises NearTie when two neighbours up to the first dropped one are closer than MARGIN but not tied."""
    values = np.asarray(values, np.float64)
    index = np.asarray(index)
    order = sorted(range(len(values)), key=lambda i: (-values[i], index[i]))
    # near-equal neighbours (float64 rounding of equal sums) are ordered by index
    i = 0
    while i < len(order):
        j = i
        while j + 1 < len(order) and np.isfinite(values[order[j + 1]]) and values[order[j]] - values[order[j + 1]] <= TIE:
            j += 1
        if j > i:
            order[i:j + 1] = sorted(order[i:j + 1], key=lambda q: index[q])
        i = j + 1
    for a, b in zip(order[:n], order[1:n + 1]):
        va, vb = values[a], values[b]
        if np.isfinite(va) and np.isfinite(vb) and va > GATED and vb > GATED and TIE < va - vb < MARGIN:
            raise NearTie("near-tie %.3g between %r and %r" % (va - vb, va, vb))
    return order[:n]


def greater(a, b):
    """a > b with the same tie / margin rule."""
    if b <= GATED or a <= GATED:
        return a > b
    if abs(a - b) <= TIE:
        return False
    if abs(a - b) < MARGIN:
        raise NearTie("near-tie %.3g in the heuristic" % (a - b))
    return a > b


def reference(script, B, K, max_length, images=None, min_length=0, length_penalty=1.0, early_stopping=False, num_return=1, pad=0,
              start=0):
    """Stock beam search over the script, float64.  Returns a dict:
      steps   per step: next_ids [B*K], beam_idx [B*K] (flat rows image * K + beam), cont (the loop condition after the step)
      sequences [B*num_return][1 + n] (n = the longest returned hypothesis), scores [B*num_return], beam_indices
      [B*num_return][n], token_scores [B*num_return][n] (0 past a hypothesis' length)"""
    eos, V = script.eos, script.V
    images = list(range(B)) if images is None else list(images)
    keep = 2 * K
    fill = pad if pad else eos                                 # utils.py:3319, `pad_token_id or eos`
    run_seq = np.full((B, K, max_length), fill, np.int64)
    run_seq[:, :, 0] = start
    seqs = run_seq.copy()
    run_sc = np.zeros((B, K))
    run_sc[:, 1:] = -1e9
    beam_sc = np.full((B, K), -1e9)
    is_fin = np.zeros((B, K), bool)
    heur = np.ones(B, bool)
    run_bi = np.full((B, K, max_length - 1), -1, np.int64)
    bi = run_bi.copy()
    run_lp = np.zeros((B, K, max_length - 1))
    lp_out = run_lp.copy()
    cur_len = 1
    steps = []
    while True:
        all_hit = True
        for b in range(B):
            cv, ci, cl = [], [], []
            for k in range(K):
                toks, lp = script.log_probs(images[b], run_seq[b, k, :cur_len], cur_len < min_length)
                cv.append(run_sc[b, k] + lp)
                ci.append(k * V + toks)
                cl.append(lp)
            cv, ci, cl = np.concatenate(cv), np.concatenate(ci), np.concatenate(cl)
            top = select(cv, ci, keep)
            topv, topi, toplp = cv[top], ci[top], cl[top]
            src, tok = topi // V, topi % V
            top_seq = run_seq[b, src].copy()
            top_seq[:, cur_len] = tok
            top_bi = run_bi[b, src].copy()
            top_bi[:, cur_len - 1] = src + b * K
            top_lp = run_lp[b, src].copy()
            top_lp[:, cur_len - 1] = toplp
            hits = (tok == eos) | (cur_len + 1 >= max_length)
            all_hit = all_hit and bool(hits.all())
            runlp = topv + hits * -1.0e9
            nxt = select(runlp, np.arange(keep), K)
            just = hits & (np.arange(keep) < K)
            fin = topv / (cur_len ** length_penalty)
            fin = fin + float(bool(is_fin[b].all()) and early_stopping is True) * -1.0e9
            fin = fin + float(not heur[b]) * -1.0e9
            fin = fin + (~just) * -1.0e9
            m_sc = np.concatenate([beam_sc[b], fin])
            sel = select(m_sc, np.arange(K + keep), K)
            m_seq = np.concatenate([seqs[b], top_seq])
            m_bi = np.concatenate([bi[b], top_bi])
            m_lp = np.concatenate([lp_out[b], top_lp])
            m_fin = np.concatenate([is_fin[b], just])
            seqs[b], beam_sc[b], bi[b], lp_out[b], is_fin[b] = m_seq[sel], m_sc[sel], m_bi[sel], m_lp[sel], m_fin[sel]
            run_seq[b], run_sc[b], run_bi[b], run_lp[b] = top_seq[nxt], runlp[nxt], top_bi[nxt], top_lp[nxt]
        cur_len += 1
        for b in range(B):                                     # utils.py:3008-3053 with the incremented cur_len
            best = run_sc[b, 0] / ((cur_len - 1) ** length_penalty)
            worst = beam_sc[b].min()
            heur[b] = heur[b] and any(greater(best, worst if f else -1.0e9) for f in is_fin[b])
        cont = bool(heur.any()) and not (bool(is_fin.all()) and early_stopping is True) and not all_hit
        steps.append(dict(next_ids=run_seq[:, :, cur_len - 1].reshape(-1).copy(), beam_idx=run_bi[:, :, cur_len - 2].reshape(-1).copy(),
                          cont=cont))
        if not cont:
            break
    nr = num_return
    out_bi = bi[:, :nr].reshape(B * nr, -1)
    n = int((out_bi != -1).sum(axis=1).max())
    return dict(steps=steps, sequences=seqs[:, :nr].reshape(B * nr, -1)[:, :1 + n], scores=beam_sc[:, :nr].reshape(-1),
                beam_indices=out_bi[:, :n], token_scores=np.where(out_bi[:, :n] != -1, lp_out[:, :nr].reshape(B * nr, -1)[:, :n], 0.0))
