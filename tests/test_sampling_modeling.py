"""generate(do_sample=True) on the Hugging Face surface (markushgrapher_amd/modeling.py), on the pattern of tests/test_modeling.py."""
import numpy as np
import pytest
import torch

from tests.conftest import load_golden
from tests.test_modeling import _e1_checkpoint_tensors, tiny_model


def _kw(g, dev):
    return {k: torch.from_numpy(g[k]).to(dev) for k in ("input_ids", "bbox", "attention_mask", "pixel_values")}


def test_sampling_argument_errors_come_before_the_device_is_needed():
    m, shape = tiny_model()
    g = load_golden("g3_trained_tiny.npz")
    kw = _kw(g, "cpu")
    with pytest.raises(ValueError, match="beam-sample"):
        m.generate(**kw, do_sample=True, num_beams=5, max_length=8)
    with pytest.raises(ValueError, match="temperature"):
        m.generate(**kw, do_sample=True, temperature=-1.0, max_length=8)
    with pytest.raises(ValueError, match="temperature"):
        m.generate(**kw, do_sample=True, temperature=0.0, max_length=8)
    with pytest.raises(ValueError, match="top_k"):
        m.generate(**kw, do_sample=True, top_k=-3, max_length=8)
    with pytest.raises(ValueError, match="top_p"):
        m.generate(**kw, do_sample=True, top_p=1.5, max_length=8)
    with pytest.raises(ValueError, match="top_p"):
        m.generate(**kw, do_sample=True, top_p=0.0, max_length=8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # valid arguments: the call reaches the engine
        m.generate(**kw, do_sample=True, max_length=8)
    # the greedy surface keeps its own rule
    with pytest.raises(ValueError, match="num_return_sequences"):
        m.generate(**kw, num_return_sequences=2, max_length=8)


@pytest.mark.gpu
def test_do_sample_shapes_seeds_and_ordering():
    m, shape = tiny_model()
    m = m.to("cuda")
    g = load_golden("g3_trained_tiny.npz")
    kw = _kw(g, m.device)
    B, T = g["input_ids"].shape[0], int(g["max_length"])
    skw = dict(do_sample=True, temperature=2.0, top_k=0, max_length=T, min_length=T)      # hot and unfiltered: the trained model's rows differ
    ids = m.generate(**kw, **skw)
    assert ids.shape == (B, T) and ids.dtype == torch.int64
    assert bool((ids[:, 0] == shape.decoder_start_token_id).all())
    # torch.manual_seed makes a sequence of calls reproducible; consecutive calls differ
    torch.manual_seed(1234)
    a1, a2 = m.generate(**kw, **skw), m.generate(**kw, **skw)
    torch.manual_seed(1234)
    b1, b2 = m.generate(**kw, **skw), m.generate(**kw, **skw)
    assert torch.equal(a1, b1) and torch.equal(a2, b2)
    assert not torch.equal(a1, a2)
    # an explicit seed is used as given, whatever torch's generator holds
    c1 = m.generate(**kw, seed=99, **skw)
    torch.manual_seed(5)
    assert torch.equal(c1, m.generate(**kw, seed=99, **skw))
    # num_return_sequences: the samples of an image are consecutive, sample j of image b draws on stream b * n + j
    n = 3
    many = m.generate(**kw, seed=99, num_return_sequences=n, **skw)
    assert many.shape == (B * n, T)
    for j in range(n):
        one = m.generate(**kw, seed=99, stream_ids=np.arange(B) * n + j, **skw)
        assert torch.equal(many[j::n], one), j
    assert not torch.equal(many[0::n], many[1::n])
    # greedy-equivalent parameters give the greedy ids
    ref = m.generate(**kw, max_length=T)
    k1 = m.generate(**kw, do_sample=True, top_k=1, max_length=T)
    assert torch.equal(k1, ref)
    assert np.array_equal(ref.cpu().numpy(), g["greedy_ids"][:, :ref.shape[1]])


@pytest.mark.gpu
def test_top_k_default_comes_from_generation_config():
    m, shape = tiny_model()
    m = m.to("cuda")
    g = load_golden("g3_trained_tiny.npz")
    kw = _kw(g, m.device)
    T = int(g["max_length"])
    skw = dict(do_sample=True, temperature=3.0, max_length=T, min_length=T, seed=7)
    ref = m.generate(**kw, max_length=T, min_length=T)

    class _GC:
        top_k = 1
    old = getattr(m, "generation_config", None)
    m.generation_config = _GC()
    try:
        assert torch.equal(m.generate(**kw, **skw), ref), "generation_config.top_k = 1 is greedy"
        assert not torch.equal(m.generate(**kw, top_k=0, **skw), ref), "an explicit top_k overrides it"
    finally:
        m.generation_config = old
    # without one: stock's default of 50
    m.generation_config = None
    try:
        assert torch.equal(m.generate(**kw, **skw), m.generate(**kw, top_k=50, **skw))
        assert not torch.equal(m.generate(**kw, **skw), m.generate(**kw, top_k=2, **skw))
    finally:
        m.generation_config = old


@pytest.mark.gpu
def test_generate_output_token_scores_and_captured_scores():
    m, shape = tiny_model()
    m = m.to("cuda")
    g = load_golden("g3_trained_tiny.npz")
    kw = _kw(g, m.device)
    B, T, temp = g["input_ids"].shape[0], int(g["max_length"]), 1.5
    out = m.generate(**kw, do_sample=True, temperature=temp, top_k=0, seed=3, max_length=T, num_return_sequences=2,
                     return_dict_in_generate=True, output_scores=True, output_logits=True)
    ids, ts = out.sequences, out.token_scores
    assert ids.shape[0] == 2 * B and ts.shape == (2 * B, ids.shape[1] - 1)
    assert torch.equal(ids, m.generate(**kw, do_sample=True, temperature=temp, top_k=0, seed=3, max_length=T, num_return_sequences=2))
    assert len(out.scores) == len(out.logits) == ids.shape[1] - 1
    eos = shape.eos_token_id
    for t in range(ids.shape[1] - 1):
        assert torch.allclose(out.scores[t], out.logits[t] / temp)
        lp = torch.log_softmax(out.scores[t].double(), -1).gather(1, ids[:, t + 1:t + 2])[:, 0]
        live = torch.ones(2 * B, dtype=torch.bool, device=ids.device)
        for r in range(2 * B):
            e = (ids[r, 1:t + 1] == eos).nonzero()
            live[r] = len(e) == 0
        assert torch.allclose(ts[live, t].double(), lp[live], atol=1e-4)
        assert bool((ts[~live, t] == 0).all())


@pytest.mark.gpu
def test_do_sample_with_the_e1_branch_attached_and_with_e1_tokens():
    m, shape = tiny_model()
    s1, sd1, extra, over = _e1_checkpoint_tensors()
    m.config.architecture_variant = "me-lf-stack-1"
    m.config.e1 = over
    sd = dict(m.state_dict()); sd.update(extra)
    m.load_state_dict(sd)
    m = m.to(torch.device("cuda:0"))
    g = load_golden("g3_trained_tiny.npz")
    kw = _kw(g, m.device)
    T = int(g["max_length"])
    skw = dict(do_sample=True, temperature=1.5, top_k=40, top_p=0.95, seed=11, num_return_sequences=2, max_length=T)
    own = m.generate(**kw, **skw)
    e1 = m._eng()._e1_engine.encode(kw["pixel_values"])
    pre = m.generate(**kw, e1=e1, **skw)
    assert torch.equal(own, pre)
    assert torch.equal(m.generate(**kw, do_sample=True, top_k=1, max_length=T), m.generate(**kw, max_length=T))
