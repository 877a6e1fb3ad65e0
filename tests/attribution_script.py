"""The attribution map restated in float64 on top of the oracle (oracle/udop_oracle.py stays as it is):

    p[l, h, b, t, k] = softmax over the attended keys of (q . k)      the decoder's cross-attention: no scale, no bias
    A[b, t, k]       = mean over the selected layers and all heads of p;  rows with decoder_attention_mask == 0 are 0

AttrOracle records softmax(scores + key mask) in float64 whenever Oracle.attention is called with bias None - that is the cross-attention
call (encoder and decoder self-attention always carry a bias).  The key axis is the oracle's own: [e1 tokens | text L | kept patches, then
the empty visual slots].  image_pooling() undoes the encoder's input assembly (Oracle.combine) with plain loops."""
import numpy as np
import torch

from oracle.udop_oracle import Oracle, _t


class AttrOracle(Oracle):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.rec = None

    def attention(self, q, k, v, bias, keymask_add):
        if bias is None and self.rec is not None:
            s = q.double() @ k.double().transpose(2, 3)
            self.rec.append(torch.softmax(s + keymask_add.double(), dim=-1))          # [B, H, T, S]
        return super().attention(q, k, v, bias, keymask_add)

    def cross_attentions(self, input_ids, bbox, pixel_values, attention_mask, decoder_input_ids, decoder_attention_mask=None, e1=None):
        """-> per decoder layer the float64 cross-attention probabilities [B, H, T, M_e1 + L + P]"""
        self.rec = []
        try:
            with torch.no_grad():
                self.forward(input_ids, bbox, pixel_values, attention_mask, decoder_input_ids=decoder_input_ids,
                             decoder_attention_mask=decoder_attention_mask, e1=e1)
            return [r.numpy() for r in self.rec]
        finally:
            self.rec = None

    def attribute(self, input_ids, bbox, pixel_values, attention_mask, decoder_input_ids, decoder_attention_mask=None, layers=None, e1=None):
        """-> A [B, T, M_e1 + L + P] float64; layers = (first, last) inclusive or None"""
        p = self.cross_attentions(input_ids, bbox, pixel_values, attention_mask, decoder_input_ids, decoder_attention_mask, e1)
        first, last = (0, len(p) - 1) if layers is None else layers
        sel = p[first:last + 1]
        a = np.zeros_like(sel[0][:, 0])
        for pl in sel:                                   # layers ascending, heads ascending
            for h in range(pl.shape[1]):
                a += pl[:, h]
        a /= len(sel) * sel[0].shape[1]
        if decoder_attention_mask is not None:
            a = a * (np.asarray(decoder_attention_mask)[..., None] != 0)
        return a


def image_pooling(shape, bbox, attention_mask, text, visual):
    """text [B, T, L], visual [B, T, P] shares -> (image [B, T, g, g], kept patches per image [B]).  Visual slot j is the j-th kept patch
    in ascending grid order; every token drops the patch its box centre falls into (stock modeling_udop.py:171-251, the 'drop for every
    token' quirk included); an attended token outside the target segment (box mean neither 0 nor 1) had that patch's embedding added to its
    own, so its share goes to that cell."""
    g = shape.image_size // shape.patch_size
    bbox = _t(bbox).to(torch.float32)
    px = torch.clip(torch.floor((bbox[:, :, 0] + bbox[:, :, 2]) / 2.0 * g).long(), 0, g - 1).numpy()
    py = torch.clip(torch.floor((bbox[:, :, 1] + bbox[:, :, 3]) / 2.0 * g).long(), 0, g - 1).numpy()
    mean = bbox.to(torch.float64).mean(-1).numpy()
    B, T, L = text.shape
    img = np.zeros((B, T, g, g), np.float64)
    kept = np.zeros(B, np.int64)
    for b in range(B):
        keep = np.ones((g, g), bool)
        for l in range(L):
            keep[py[b, l], px[b, l]] = False
        j = 0
        for y in range(g):
            for x in range(g):
                if keep[y, x]:
                    img[b, :, y, x] += visual[b, :, j]
                    j += 1
        kept[b] = j
        for l in range(L):
            attended = attention_mask is None or attention_mask[b, l] != 0
            if attended and mean[b, l] != 0.0 and mean[b, l] != 1.0:
                img[b, :, py[b, l], px[b, l]] += text[b, :, l]
    return img, kept
