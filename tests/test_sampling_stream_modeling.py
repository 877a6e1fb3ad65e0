"""generate_queue(do_sample=True) on the Hugging Face surface (markushgrapher_amd/modeling.py): the sampled queue against the per-image loop
`model.generate(**encoding, do_sample=True, stream_ids=...)`, on the pattern of tests/test_sampling_modeling.py."""
import json
import os

import numpy as np
import pytest
import torch

from tests.conftest import load_golden
from tests.test_modeling import GOLDEN, tiny_model

SKW = dict(temperature=1.5, top_k=0, max_length=16)      # hot and unfiltered: the trained model's rows differ and end at different steps


def _encodings(n=7):
    """Per-sample encodings of DIFFERENT text lengths, as the reference's evaluation loop builds them."""
    with open(os.path.join(GOLDEN, "pipeline_host.json")) as f:
        pages = json.load(f)["pages"]
    g = load_golden("g3_trained_tiny.npz")
    out = []
    for k in range(n):
        p = pages[k % len(pages)]
        out.append({"input_ids": torch.tensor([p["input_ids"]]), "bbox": torch.tensor([p["bbox"]], dtype=torch.float32),
                    "pixel_values": torch.from_numpy(g["pixel_values"][k % g["pixel_values"].shape[0]][None])})
    return out


def test_sampled_queue_argument_errors_come_before_the_device_is_needed():
    m, shape = tiny_model()
    encs = _encodings(2)
    with pytest.raises(ValueError, match="beam-sample"):
        m.generate_queue(encs, do_sample=True, num_beams=5, max_length=8)
    with pytest.raises(ValueError, match="temperature"):
        m.generate_queue(encs, do_sample=True, temperature=0.0, max_length=8)
    with pytest.raises(ValueError, match="top_k"):
        m.generate_queue(encs, do_sample=True, top_k=-3, max_length=8)
    with pytest.raises(ValueError, match="top_p"):
        m.generate_queue(encs, do_sample=True, top_p=1.5, max_length=8)
    with pytest.raises(ValueError, match="num_return_sequences"):      # the greedy queue keeps its own rule
        m.generate_queue(encs, num_return_sequences=2, max_length=8)


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 2])
def test_sampled_queue_equals_the_per_image_loop(S):
    """The documented contract: generate_queue(encs, do_sample=True, seed=s, **w)[n] == generate(**encs[n], do_sample=True, seed=s,
    stream_ids=[n * S .. n * S + S - 1], num_return_sequences=S, **w) cut at its length; and contexts=2 == contexts=1."""
    m, shape = tiny_model()
    m = m.to("cuda")
    dev = m.device
    encs = _encodings(7)
    loop = []
    for n, e in enumerate(encs):
        enc = {k: v.to(dev) for k, v in e.items()}
        out = m.generate(**enc, do_sample=True, seed=31, stream_ids=np.arange(n * S, n * S + S), num_return_sequences=S,
                         return_dict_in_generate=True, **SKW)
        loop.append((out.sequences.cpu(), out.token_scores.cpu()))
    got = m.generate_queue(encs, do_sample=True, seed=31, num_return_sequences=S, slots=3, chunk=2, **SKW)
    assert len(got) == len(encs)
    eos, pad = shape.eos_token_id, shape.pad_token_id
    for n, (seqs, ts) in enumerate(loop):
        if S == 1:
            assert got[n].dim() == 1
            b = seqs[0].tolist()
            cut = b.index(eos) + 1 if eos in b[1:] else len(b)
            assert got[n].cpu().tolist() == b[:cut], n
        else:
            d = got[n]
            assert d["sequences"].shape[0] == S and d["token_scores"].shape == (S, d["sequences"].shape[1] - 1)
            assert torch.equal(d["sequences"].cpu(), seqs), n       # both are [S, the longest sample's columns], pad after a row's EOS
            assert torch.equal(d["token_scores"].cpu(), ts), n
    rows = [tuple(g.cpu().tolist()) if S == 1 else tuple(g["sequences"].cpu().reshape(-1).tolist()) for g in got]
    assert len(set(rows)) > 1
    if S == 1:
        assert len({len(r) for r in rows}) > 1, "the rows end at different steps"
        scored = m.generate_queue(encs, do_sample=True, seed=31, return_scores=True, slots=3, chunk=2, **SKW)
        for n, d in enumerate(scored):
            assert d["sequences"].shape[0] == 1 and d["sequences"][0].cpu().tolist() == list(rows[n])
            assert torch.equal(d["token_scores"][0].cpu(), loop[n][1][0][:len(rows[n]) - 1])
    two = m.generate_queue(encs, do_sample=True, seed=31, num_return_sequences=S, slots=3, chunk=2, contexts=2, **SKW)
    assert getattr(m, "_inflight", None) is not None and len(m._inflight) == 2
    for a, b in zip(got, two):
        if S == 1:
            assert torch.equal(a, b)
        else:
            assert torch.equal(a["sequences"], b["sequences"]) and torch.equal(a["token_scores"], b["token_scores"])
    m._inflight.close()


@pytest.mark.gpu
def test_sampled_queue_seeds():
    m, shape = tiny_model()
    m = m.to("cuda")
    encs = _encodings(5)
    kw = dict(do_sample=True, slots=3, chunk=2, min_length=16, **SKW)       # no early stop: every column is a draw
    with pytest.raises(ValueError, match="beam-sample"):
        m.generate_queue(encs, num_beams=5, **kw)

    def rows(**over):
        return torch.stack(m.generate_queue(encs, **dict(kw, **over))).cpu()

    torch.manual_seed(1234)
    a1, a2 = rows(), rows()
    torch.manual_seed(1234)
    b1, b2 = rows(), rows()
    assert torch.equal(a1, b1) and torch.equal(a2, b2)
    assert not torch.equal(a1, a2)
    c1 = rows(seed=99)
    torch.manual_seed(5)
    assert torch.equal(c1, rows(seed=99))
    # greedy-equivalent options give the greedy queue
    ref = m.generate_queue(encs, max_length=16, slots=3, chunk=2)
    k1 = m.generate_queue(encs, do_sample=True, top_k=1, max_length=16, slots=3, chunk=2)
    assert all(torch.equal(a, b) for a, b in zip(ref, k1))
