"""MarkushgrapherForConditionalGeneration.score(): the HF-style surface over Engine.score / Engine.score_candidates.

  loss               = forward(labels=...).loss within 1e-3, with -100 positions present (the same decoder stack and logits; the fused path sums
                       fp32 log-probabilities in float64, cross_entropy reduces fp32 logits in fp32: errors of 1e-6 per position)
  sequence_logprobs  = the masked sum of token_logprobs; [B, C, T] labels give [B, C]
  argmax_ids         reproduce the reference evaluation's accuracy count (argmax of the logits against the labels up to the last EOS label,
                     core/trainers/curriculumTrainer.py:654-672), sample by sample as the reference runs it"""
import numpy as np
import pytest
import torch

from tests.conftest import load_golden
from tests.test_modeling import tiny_model


def _model_and_batch():
    m, shape = tiny_model()
    m = m.to("cuda")
    g = load_golden("g3_trained_tiny.npz")
    kw = {k: torch.from_numpy(g[k]).to(m.device) for k in ("input_ids", "bbox", "attention_mask", "pixel_values")}
    labels = torch.from_numpy(g["labels"]).to(m.device)
    return m, shape, g, kw, labels


def test_score_needs_labels():
    m, _ = tiny_model()
    with pytest.raises(ValueError, match="labels"):
        m.score(None, None, None)


@pytest.mark.gpu
def test_loss_and_sequence_logprobs_match_forward():
    m, shape, g, kw, labels = _model_and_batch()
    assert bool((labels == -100).any())              # the fixture's labels carry ignored positions
    out = m.score(**kw, labels=labels)
    fwd = m(**kw, labels=labels)
    print("score().loss", float(out.loss), "forward().loss", float(fwd.loss))
    assert abs(float(out.loss) - float(fwd.loss)) < 1e-3
    live = labels != -100
    lp = torch.log_softmax(fwd.logits.double(), -1).gather(-1, labels.clamp(min=0)[..., None])[..., 0]
    ref_seq = torch.where(live, lp, torch.zeros_like(lp)).sum(-1)
    assert out.token_logprobs.shape == labels.shape and out.sequence_logprobs.shape == labels.shape[:1]
    assert torch.all(out.token_logprobs[~live] == 0)
    assert torch.equal(out.sequence_logprobs, out.token_logprobs.sum(-1))          # ignored positions hold 0.0: the plain sum is the masked sum
    assert float((out.sequence_logprobs.double() - ref_seq).abs().max()) < 1e-3 * labels.shape[1]
    assert float((out.token_logprobs.double() - torch.where(live, lp, torch.zeros_like(lp))).abs().max()) < 1e-3
    # explicit decoder_input_ids = the default
    out2 = m.score(**kw, labels=labels, decoder_input_ids=m._shift_right(labels))
    assert torch.equal(out2.token_logprobs, out.token_logprobs) and torch.equal(out2.argmax_ids, out.argmax_ids)


@pytest.mark.gpu
def test_candidate_labels_give_per_candidate_scores():
    m, shape, g, kw, labels = _model_and_batch()
    other = labels.roll(1, 0)
    cand = torch.stack([labels, other, labels], 1)                                 # [B, 3, T]
    out = m.score(**kw, labels=cand)
    B, T = labels.shape
    assert out.token_logprobs.shape == (B, 3, T) and out.sequence_logprobs.shape == (B, 3) and out.argmax_ids.shape == (B, 3, T)
    one = m.score(**kw, labels=labels)
    assert torch.equal(out.token_logprobs[:, 0], one.token_logprobs) and torch.equal(out.token_logprobs[:, 2], one.token_logprobs)
    assert torch.equal(out.sequence_logprobs[:, 0], one.sequence_logprobs)
    # the trained fixture prefers an image's own labels to its neighbour's
    differ = (labels != other).any(1)
    assert bool(differ.any()) and torch.all(out.sequence_logprobs[differ, 0] > out.sequence_logprobs[differ, 1])
    n = (cand != -100).sum()
    assert abs(float(out.loss) + float(out.token_logprobs.double().sum() / n)) < 1e-6


@pytest.mark.gpu
def test_argmax_ids_reproduce_the_reference_accuracy():
    m, shape, g, kw, labels = _model_and_batch()
    eos = shape.eos_token_id

    def accuracy(pred, label):
        """correct / total predictions up to (and including) the last EOS label of the batch, as the reference's evaluation loop counts them"""
        at = (label == eos).nonzero(as_tuple=False)
        last = int(at.max()) if at.numel() else label.size(1)
        p, l = pred[:, :last + 1], label[:, :last + 1]
        return int((p == l).sum()), p.numel()

    got, want = [0, 0], [0, 0]
    for b in range(labels.shape[0]):                 # the reference evaluates sample by sample
        one = {k: v[b:b + 1] for k, v in kw.items()}
        lab = labels[b:b + 1]
        c, t = accuracy(m.score(**one, labels=lab).argmax_ids, lab)
        got[0] += c; got[1] += t
        c, t = accuracy(torch.argmax(m(**one, labels=lab).logits, dim=2), lab)
        want[0] += c; want[1] += t
    assert got == want and got[1] > 0 and got[0] > 0
