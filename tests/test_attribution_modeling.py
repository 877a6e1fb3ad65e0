"""MarkushgrapherForConditionalGeneration.attribute(): the HF-style surface over Engine.attribute / Engine.attribute_candidates on the trained
tiny fixture.  On the emulator the model's engine is replaced by one over the CPU backend, as tests/test_decoder_prompt_modeling.py does.

  sequences    what generate() returned reproduces the labels-driven output for the same tokens; `valid` ends at the first EOS
  identity     image.sum + (share of the text tokens that received no patch) + e1.sum = 1 on valid rows
  assembly     the kept patches per image that the pooling derives from bbox = enc_mask[:, L:].sum() of the engine (the device assembly)
  pooling      `image` against the loops of tests/attribution_script.image_pooling
  arguments    both or neither of sequences / labels, bad layers; on the CPU without a library the "no CPU fallback" error"""
import numpy as np
import pytest
import torch

from markushgrapher_amd import synth
from markushgrapher_amd.modeling import AttributionOutput, patch_assignment
from tests.attribution_script import image_pooling
from tests.backends import make_engine
from tests.conftest import load_golden
from tests.test_modeling import tiny_model
from tests.test_oracle_golden import _weights

BACKENDS = [pytest.param("emu"), pytest.param("hip", marks=pytest.mark.gpu)]
T = 16


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


@pytest.fixture
def case(request, monkeypatch):
    be_name = request.param
    m, shape = tiny_model()
    g = load_golden("g3_trained_tiny.npz")
    dev = "cpu"
    if be_name == "hip":
        m = m.to("cuda")
        dev = m.device
    else:
        eng = make_engine("emu", *_weights(g))
        monkeypatch.setattr(m, "_eng", lambda: eng)
    kw = {k: torch.from_numpy(g[k]).to(dev) for k in ("input_ids", "bbox", "attention_mask", "pixel_values")}
    return m, shape, kw, g


@pytest.mark.parametrize("case", BACKENDS, indirect=True)
def test_sequences_reproduce_labels(case):
    m, shape, kw, g = case
    seq = m.generate(**kw, max_length=T)
    seq = seq if torch.is_tensor(seq) else torch.from_numpy(_np(seq))
    out = m.attribute(**kw, sequences=seq)
    assert isinstance(out, AttributionOutput)
    B, L = kw["input_ids"].shape
    gsz = shape.image_size // shape.patch_size
    assert out.cross_attention.shape == (B, seq.shape[1] - 1, L + gsz * gsz) and out.e1 is None
    assert out.text.shape == (B, seq.shape[1] - 1, L) and out.image.shape == (B, seq.shape[1] - 1, gsz, gsz)
    s = _np(seq)
    valid = _np(out.valid)
    assert bool((s[:, 1:] == shape.eos_token_id).any()), "the trained fixture ends its sequences"
    for b in range(B):
        e = np.flatnonzero(s[b, 1:] == shape.eos_token_id)
        n = int(e[0]) + 1 if len(e) else s.shape[1] - 1
        assert valid[b, :n].all() and not valid[b, n:].any()          # row t explains s[b, t + 1]; the EOS row is the last valid one
    # the same tokens as labels: -100 after the EOS
    labels = torch.from_numpy(np.where(valid, s[:, 1:], -100)).to(seq.device)
    ref = m.attribute(**kw, labels=labels)
    assert np.array_equal(_np(ref.valid), valid)
    a, r = _np(out.cross_attention), _np(ref.cross_attention)
    assert np.all(a[~valid] == 0.0) and np.all(r[~valid] == 0.0)
    # (labels: pad tokens follow the EOS as decoder inputs, unmasked; a valid row never looks at them - causal - so the bits agree)
    assert np.array_equal(a.view(np.uint32), r.view(np.uint32))
    assert np.array_equal(_np(out.image).view(np.uint32), _np(ref.image).view(np.uint32))
    assert np.abs(a.astype(np.float64).sum(-1)[valid] - 1).max() <= 1e-5
    # n-best / samples: [B, C, T + 1]
    cand = torch.stack([seq, seq.roll(1, 0)], 1)
    oc = m.attribute(**kw, sequences=cand, layers=(0, 1))
    assert oc.cross_attention.shape == (B, 2) + tuple(out.cross_attention.shape[1:]) and oc.image.shape == (B, 2) + tuple(out.image.shape[1:])
    assert np.array_equal(_np(oc.cross_attention[:, 0]).view(np.uint32), a.view(np.uint32))
    assert np.array_equal(_np(oc.image[:, 0]).view(np.uint32), _np(out.image).view(np.uint32))
    assert np.array_equal(_np(oc.valid[:, 1]), np.roll(valid, 1, 0))


@pytest.mark.parametrize("case", BACKENDS, indirect=True)
@pytest.mark.parametrize("with_e1", [False, True])
def test_sum_identity_and_pooling(case, with_e1):
    m, shape, kw, g = case
    labels = torch.from_numpy(np.asarray(g["labels"]).astype(np.int64)).to(kw["input_ids"].device)
    B, L = kw["input_ids"].shape
    M = 5 if with_e1 else 0
    e1 = None
    if with_e1:
        e1 = torch.from_numpy(synth.round_bf16(synth.uniform_pm1("e1.tokens", (B, M, shape.d_model), 2) * np.float32(1.5))).to(labels.device)
    out = m.attribute(**kw, labels=labels, e1=e1, layers=1)
    gsz = shape.image_size // shape.patch_size
    valid = _np(out.valid)
    assert np.array_equal(valid, _np(labels) != -100) and bool((~valid).any())
    assert (out.e1 is None) == (not with_e1)
    if with_e1:
        assert out.e1.shape == (B, labels.shape[1], M) and out.cross_attention.shape[-1] == M + L + gsz * gsz
    # the device assembly: kept patches per image
    pts, recv, keep = patch_assignment(kw["bbox"], kw["attention_mask"], gsz)
    eng = m._eng()
    enc_mask = _np(eng.encode(kw["input_ids"], kw["bbox"], kw["attention_mask"], kw["pixel_values"])[1])
    assert np.array_equal(_np(keep.sum(1)), enc_mask[:, L:].sum(1))
    assert bool((~recv).any()) and bool(recv.any())           # the fixture has receiving and non-receiving text tokens
    # the identity
    text, img = _np(out.text).astype(np.float64), _np(out.image).astype(np.float64)
    no_patch = (text * (~_np(recv))[:, None, :]).sum(-1)
    total = img.sum((-1, -2)) + no_patch + (_np(out.e1).astype(np.float64).sum(-1) if with_e1 else 0.0)
    assert np.abs(total[valid] - 1).max() <= 1e-5
    assert np.all(total[~valid] == 0.0)
    # the pooling against the plain loops
    vis = _np(out.cross_attention)[..., M + L:].astype(np.float64)
    ref_img, kept = image_pooling(shape, _np(kw["bbox"]), _np(kw["attention_mask"]), text, vis)
    assert np.array_equal(kept, enc_mask[:, L:].sum(1))
    assert np.abs(img - ref_img).max() <= 1e-6
    assert img[valid].max() > 0.05


def test_arguments_are_validated():
    m, shape = tiny_model()
    z = torch.zeros(1, 4, dtype=torch.long)
    with pytest.raises(ValueError, match="exactly one"):
        m.attribute(None, None, None)
    with pytest.raises(ValueError, match="exactly one"):
        m.attribute(None, None, None, sequences=z, labels=z)
    for bad in (-1, 2, (1, 0), (0, 2), (0,), "all", (0.0, 1.0)):
        with pytest.raises(ValueError, match="layers"):
            m.attribute(None, None, None, labels=z, layers=bad)
    # on the CPU there is no library behind the model: the error every entry point raises
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.attribute(z, torch.zeros(1, 4, 4), torch.zeros(1, 3, shape.image_size, shape.image_size), sequences=z)
