"""CPU: the float64 restatement of tests/attribution_script.py pinned to stock transformers - UdopForConditionalGeneration(...,
output_attentions=True).cross_attentions, one [B, H, T, S] tensor per decoder layer - on the g0_tiny and g3_trained_tiny fixtures, for the
full layer range and a single layer.  Both sides are the fp32 model; the restatement's softmax is float64, stock's fp32: 1e-5."""
import numpy as np
import pytest
import torch

from tests.attribution_script import AttrOracle
from tests.conftest import load_golden
from tests.test_oracle_golden import _inputs, _weights


@pytest.mark.parametrize("fixture", ["g0_tiny.npz", "g3_trained_tiny.npz"])
def test_restatement_equals_stock_cross_attentions(fixture):
    pytest.importorskip("transformers", reason="stock transformers is not installed")
    from tools.stock import stock_model
    g = load_golden(fixture)
    shape, sd = _weights(g)
    inp = _inputs(g, shape)
    labels = np.asarray(g["labels"]).astype(np.int64)
    o = AttrOracle(shape, sd)
    dec = o.shift_right(labels, shape.decoder_start_token_id, shape.pad_token_id)
    dam = (labels != -100).astype(np.int64)
    m = stock_model(shape, sd)
    with torch.no_grad():
        out = m(input_ids=torch.from_numpy(np.asarray(inp["input_ids"])).long(), bbox=torch.from_numpy(np.asarray(inp["bbox"])).float(),
                attention_mask=torch.from_numpy(np.asarray(inp["attention_mask"])).long(),
                pixel_values=torch.from_numpy(np.asarray(inp["pixel_values"])).float(), decoder_input_ids=dec,
                decoder_attention_mask=torch.from_numpy(dam), output_attentions=True, return_dict=True)
    xa = [a.double().numpy() for a in out.cross_attentions]
    assert len(xa) == shape.num_decoder_layers and xa[0].shape[1] == shape.num_heads
    args = (inp["input_ids"], inp["bbox"], inp["pixel_values"], inp["attention_mask"], dec.numpy(), dam)
    rec = o.cross_attentions(*args)
    for l, (a, r) in enumerate(zip(xa, rec)):                # the recorded probabilities themselves, layer by layer
        assert a.shape == r.shape
        assert np.abs(a - r).transpose(0, 2, 1, 3)[dam != 0].max() <= 1e-5, l          # (rows of [B, T, H, S] under the decoder mask)
    live = dam != 0
    for layers in (None, (0, 0), (shape.num_decoder_layers - 1,) * 2):
        first, last = (0, len(xa) - 1) if layers is None else layers
        ref = np.mean([a.mean(1) for a in xa[first:last + 1]], 0) * live[..., None]
        got = o.attribute(*args, layers=layers)
        err = np.abs(got - ref).max()
        print(f"{fixture} layers {layers}: max |restatement - stock| = {err:.3e}")
        assert err <= 1e-5
        assert np.abs(got.sum(-1)[live] - 1).max() <= 1e-5 and np.all(got[~live] == 0.0)
