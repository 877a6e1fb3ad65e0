"""Decoder prompts on scripted logits: float64 restatements of stock transformers 5.15 `generate` with `input_ids` as the prompt, built on
tests/beam_script.py's Script and selection rules (value descending, index ascending; NearTie when a float32 run could order differently).

A prompt is the list of tokens an image's rows start with (prompts[b][0] is what stock calls the start token).  All images share ONE step
counter, as the device loops do: while the column being written is below an image's prompt length the step only appends the prompt's
token; from there on the image runs stock's step with decoder_prompt_len = its own prompt length (generation/utils.py::_beam_search: the
finished-score divisor (cur_len + 1 - prompt_len)^length_penalty, the early-stop heuristic's best hypothetical length cur_len - prompt_len).
An image of a ragged batch therefore computes what a stock call on it alone computes; tests/test_decoder_prompt_stock.py pins that.
"""
import numpy as np

from tests.beam_script import MARGIN, TIE, NearTie, greater, select


def greedy_reference(script, prompts, max_length, images=None, min_length=0, pad=0):
    """Stock greedy search over the script from the given prompts -> dict(sequences [B][cols] padded with `pad` after a row's EOS,
    token_scores [B][cols - 1] float64 log-softmax of the processed logits at the emitted token, 0.0 in prompt columns and after EOS)."""
    B = len(prompts)
    images = list(range(B)) if images is None else list(images)
    rows, scores = [], []
    for b in range(B):
        seq = [int(t) for t in prompts[b]]
        sc = [0.0] * (len(seq) - 1)
        while len(seq) < max_length:
            x = script.logits(images[b], seq).astype(np.float64)
            if len(seq) < min_length:
                x[script.eos] = -np.inf
            order = np.argsort(-x, kind="stable")
            if TIE < x[order[0]] - x[order[1]] < MARGIN:
                raise NearTie("near-tie in a greedy step")
            tok = int(order[0])
            mx = x.max()
            sc.append(float(x[tok] - mx - np.log(np.exp(x - mx).sum())))
            seq.append(tok)
            if tok == script.eos:
                break
        rows.append(seq)
        scores.append(sc)
    cols = max(len(r) for r in rows)
    out = np.full((B, cols), pad, np.int64)
    ts = np.zeros((B, cols - 1))
    for b in range(B):
        out[b, :len(rows[b])] = rows[b]
        ts[b, :len(scores[b])] = scores[b]
    return dict(sequences=out, token_scores=ts)


def reference(script, B, K, max_length, prompts, images=None, min_length=0, length_penalty=1.0, early_stopping=False, num_return=1, pad=0):
    """tests/beam_script.reference with a prompt per image.  Same result dict; sequences include the prompt columns, beam_indices hold the
    image's beam-0 flat row (image * K) in forced columns, token_scores 0.0 there; `steps` lists every step, forced ones included (next_ids
    = the forced token for every beam, beam_idx = the identity)."""
    eos, V = script.eos, script.V
    images = list(range(B)) if images is None else list(images)
    plen = [len(p) for p in prompts]
    assert len(prompts) == B and all(1 <= n < max_length for n in plen)
    keep = 2 * K
    fill = pad if pad else eos
    run_seq = np.full((B, K, max_length), fill, np.int64)
    run_bi = np.full((B, K, max_length - 1), -1, np.int64)
    for b in range(B):
        run_seq[b, :, :plen[b]] = np.asarray(prompts[b], np.int64)
        run_bi[b, :, :plen[b] - 1] = b * K
    seqs = run_seq.copy()                                      # utils.py:3326-3327
    run_sc = np.zeros((B, K))
    run_sc[:, 1:] = -1e9
    beam_sc = np.full((B, K), -1e9)
    is_fin = np.zeros((B, K), bool)
    heur = np.ones(B, bool)
    bi = np.full((B, K, max_length - 1), -1, np.int64)
    run_lp = np.zeros((B, K, max_length - 1))
    lp_out = run_lp.copy()
    cur_len = 1
    steps = []
    while True:
        all_hit = True
        step_idx = np.zeros((B, K), np.int64)
        for b in range(B):
            if cur_len < plen[b]:                              # a forced column: nothing is ranked, the image goes on
                all_hit = False
                step_idx[b] = b * K + np.arange(K)
                continue
            P = plen[b]
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
            fin = topv / ((cur_len + 1 - P) ** length_penalty)                 # utils.py:3182
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
            step_idx[b] = run_bi[b, :, cur_len - 1]
        cur_len += 1
        for b in range(B):                                     # utils.py:3008-3053 with the incremented cur_len
            if cur_len <= plen[b]:
                continue
            best = run_sc[b, 0] / ((cur_len - plen[b]) ** length_penalty)
            worst = beam_sc[b].min()
            heur[b] = heur[b] and any(greater(best, worst if f else -1.0e9) for f in is_fin[b])
        cont = bool(heur.any()) and not (bool(is_fin.all()) and early_stopping is True) and not all_hit
        steps.append(dict(next_ids=run_seq[:, :, cur_len - 1].reshape(-1).copy(), beam_idx=step_idx.reshape(-1).copy(), cont=cont))
        if not cont:
            break
    nr = num_return
    out_bi = bi[:, :nr].reshape(B * nr, -1)
    n = int((out_bi != -1).sum(axis=1).max())
    return dict(steps=steps, sequences=seqs[:, :nr].reshape(B * nr, -1)[:, :1 + n], scores=beam_sc[:, :nr].reshape(-1),
                beam_indices=out_bi[:, :n], token_scores=np.where(out_bi[:, :n] != -1, lp_out[:, :nr].reshape(B * nr, -1)[:, :n], 0.0))
