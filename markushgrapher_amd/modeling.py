"""HuggingFace-style surface of the MarkushGrapher-2 VTL encoder + CXSMILES decoder on the MI355X HIP engine.

Mirrors what the reference imports from its transformers fork (`transformers.models.markushgrapher`,
ref: markushgrapher/core/common/begin.py:7-13) for THIS path, with the same names, argument meaning and outputs:

    config = MarkushgrapherConfig.from_pretrained(path); config.image_size = 512        (ref: begin.py:114-121)
    model  = MarkushgrapherForConditionalGeneration.from_pretrained(path, config=config).to(device)   (begin.py:128-133)
    ids    = model.generate(**encoding, num_beams=5, max_length=512)     (ref: utils/ocsr/utils_evaluation.py:269-285)
    logits = model(**sample).logits                                      (ref: core/trainers/curriculumTrainer.py:654-656)

The torch tensors held here are only the HF-layout copy of the weights (for state_dict()/parameters(), which the
reference's save/compare helpers walk: ref: utils/model/utils_model_loading.py:6-46) and the memory carrier of
inputs/outputs; every computation of forward()/generate() runs in the HIP library behind the C ABI.
"""
from __future__ import annotations

import json
import os
import warnings
from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np
import torch
from torch import nn

from .engine import Engine, MgError, TorchMem
from .synth import ModelShape, state_dict_spec, tied_aliases


class MarkushgrapherConfig:
    """UdopConfig-compatible field names (stock transformers models/udop/configuration_udop.py:43-71) plus the
    attributes the reference sets (`architecture_variant`, `output_attentions`, ref: begin.py:119-121)."""

    model_type = "markushgrapher"

    def __init__(self, **kw):
        base = ModelShape()
        ndl = kw.get("num_decoder_layers", None)                 # UdopConfig: defaults to num_layers when absent / None
        for k, v in base.to_dict().items():
            setattr(self, k, kw.pop(k, v))
        self.num_decoder_layers = ndl if ndl is not None else self.num_layers
        # "none" = the plain VTL encoder + decoder; "me-lf-stack-1" = MarkushGrapher-2's two-encoder late fusion, whose OCSR
        # branch (e1) this package does not compute (ref default: core/common/arguments.py:258; set at begin.py:120)
        self.architecture_variant = kw.pop("architecture_variant", "none")
        self.allow_missing_e1 = bool(kw.pop("allow_missing_e1", False))
        # geometry of the OCSR vision branch: overrides of e1_shapes.PRESETS["swin_b_384"] (MolScribe's Swin-B), e.g. {"pix_scale": [...]};
        # d_model / src_image_size follow this config, the projector's layer sizes follow the checkpoint's tensors
        self.e1 = dict(kw.pop("e1", None) or {})
        self.output_attentions = kw.pop("output_attentions", False)
        self.max_length = kw.pop("max_length", 512)
        self.tie_word_embeddings = bool(kw.pop("tie_word_embeddings", True))      # UDOP / T5 default
        self.is_encoder_decoder = True
        self.extra = kw

    @classmethod
    def from_pretrained(cls, path, **kw):
        with open(os.path.join(path, "config.json")) as f:
            d = json.load(f)
        d.update(kw)
        if isinstance(d.get("image_size"), (list, tuple)):
            d["image_size"] = d["image_size"][0]
        return cls(**d)

    def to_shape(self) -> ModelShape:
        return ModelShape(**{k: getattr(self, k) for k in ModelShape().to_dict()})

    def to_dict(self):
        d = self.to_shape().to_dict()
        d.update(architecture_variant=self.architecture_variant, model_type=self.model_type,
                 tie_word_embeddings=self.tie_word_embeddings, max_length=self.max_length)
        if self.e1:
            d["e1"] = {k: (list(v) if isinstance(v, tuple) else v) for k, v in self.e1.items()}
        return d


@dataclass
class Seq2SeqLMOutput:
    loss: Optional[torch.Tensor] = None
    logits: Optional[torch.Tensor] = None
    encoder_last_hidden_state: Optional[torch.Tensor] = None
    encoder_attention_mask: Optional[torch.Tensor] = None

    def __getitem__(self, i):
        return (self.loss, self.logits)[i] if self.loss is not None else (self.logits,)[i]


@dataclass
class ScoreOutput:
    """score(): log-probabilities of given target sequences, computed on the device without the [.., vocab] logits.
      token_logprobs     [B, T] or [B, C, T]: log_softmax(logits)[label]; 0.0 where the label is -100
      sequence_logprobs  [B] or [B, C]: the sum of a sequence's token_logprobs over its non-ignored positions
      loss               mean negative log-probability over the call's non-ignored positions (= forward(labels=...).loss)
      argmax_ids         [B, T] or [B, C, T]: the model's own prediction at every position (ties: the lowest id)
      argmax_logprobs    its log-probability"""
    token_logprobs: torch.Tensor
    sequence_logprobs: torch.Tensor
    loss: torch.Tensor
    argmax_ids: torch.Tensor
    argmax_logprobs: torch.Tensor

    def __getitem__(self, k):
        return getattr(self, k)


@dataclass
class AttributionOutput:
    """attribute(): where in the page each output token came from - the decoder's cross-attention over the given sequences, averaged over
    heads and the selected layers, computed on the device without the [B, H, T, S] probabilities.  T rows per sequence ([B, T, ..] or
    [B, C, T, ..]); row t explains the token the decoder wrote after reading decoder input t.
      cross_attention  [.., T, M_e1 + L + P] over [e1 tokens | text slots | visual slots]; unattended keys and invalid rows are 0,
                       every valid row sums to 1
      valid            [.., T] bool: rows up to and including a sequence's first EOS (sequences=) / where the label is not -100 (labels=)
      e1               [.., T, M_e1] the OCSR-branch tokens' share (None without the branch)
      text             [.., T, L] the text / OCR-cell tokens' share
      image            [.., T, g, g], g = image_size / patch_size: the page.  A kept patch's share, plus the share of every text token whose
                       embedding received that patch's embedding (an attended token outside the target segment), at the patch's grid cell.
                       image.sum((-1, -2)) + (share of the text tokens that received no patch) + e1.sum(-1) = 1 on valid rows"""
    cross_attention: torch.Tensor
    valid: torch.Tensor
    e1: Optional[torch.Tensor]
    text: torch.Tensor
    image: torch.Tensor

    def __getitem__(self, k):
        return getattr(self, k)


def patch_assignment(bbox, attention_mask, grid):
    """The encoder's input assembly (stock modeling_udop.py:171-251) restated on bbox [B, L, 4]: -> (pts [B, L] the grid cell, row-major,
    whose patch embedding a text token is offered; recv [B, L] bool, the tokens that actually receive it - attended and outside the target
    segment, i.e. the mean of the box is neither 0 nor 1; keep [B, grid * grid] bool, the patches that stay as visual slots - every token
    drops its cell, padded and target-segment tokens included)."""
    bbox = bbox.float()
    px = torch.clip(torch.floor((bbox[:, :, 0] + bbox[:, :, 2]) / 2.0 * grid).long(), 0, grid - 1)
    py = torch.clip(torch.floor((bbox[:, :, 1] + bbox[:, :, 3]) / 2.0 * grid).long(), 0, grid - 1) * grid
    pts = px + py
    mean = bbox.to(torch.float64).mean(-1)
    recv = ~((mean == 0.0) | (mean == 1.0))
    if attention_mask is not None:
        recv = recv & (attention_mask.to(bbox.device) != 0)
    keep = torch.ones(bbox.shape[0], grid * grid, dtype=torch.bool, device=bbox.device)
    keep.scatter_(1, pts, torch.zeros_like(pts, dtype=torch.bool))
    return pts, recv, keep


def pool_to_image(text, visual, pts, recv, keep, grid):
    """text [B, R, L] and visual [B, R, P] shares -> [B, R, grid, grid]: visual slot j is the j-th kept patch in ascending grid order; a
    receiving text token adds its share at its cell."""
    B, R, P = visual.shape
    slot = (keep.long().cumsum(1) - 1).clamp(min=0)                                  # kept patch -> its visual slot
    img = visual.gather(2, slot[:, None, :].expand(B, R, P)) * keep[:, None, :].to(visual.dtype)
    img = img.scatter_add(2, pts[:, None, :].expand(B, R, pts.shape[1]), text * recv[:, None, :].to(text.dtype))
    return img.view(B, R, grid, grid)


@dataclass
class GenerateOutput:
    """generate(return_dict_in_generate=True): the fields of stock GenerateEncoderDecoderOutput / GenerateBeamEncoderDecoderOutput that
    this path fills, plus `token_scores`.
      sequences         [B * num_return_sequences, T]
      sequences_scores  [B * num_return_sequences] (beam search)
      beam_indices      [B * num_return_sequences, T - 1] (beam search; -1 past a hypothesis' length)
      scores / logits   tuples of T - 1 tensors [B * num_beams, vocab] (output_scores / output_logits only; see generate())
      token_scores      [B * num_return_sequences, T - 1], computed on the device beside the ids: greedy = compute_transition_scores(
                        normalize_logits=True), beam = compute_transition_scores(beam_indices=..., normalize_logits=False); 0.0 after a
                        row's EOS / past a hypothesis' length"""
    sequences: torch.Tensor
    sequences_scores: Optional[torch.Tensor] = None
    beam_indices: Optional[torch.Tensor] = None
    scores: Optional[tuple] = None
    logits: Optional[tuple] = None
    token_scores: Optional[torch.Tensor] = None

    def __getitem__(self, k):
        return getattr(self, k)


class _ParamTree(nn.Module):
    """nn.Module tree built from dotted state-dict keys, so `.encoder.block[0]...`, `.decoder`, `.lm_head` exist with
    the HF names and carry state_dict()/parameters()."""

    def add(self, dotted: str, tensor: torch.Tensor):
        head, _, rest = dotted.partition(".")
        if not rest:
            self.register_parameter(head, nn.Parameter(tensor, requires_grad=False))
            return
        if head not in self._modules:
            self.add_module(head, _ParamTree())
        self._modules[head].add(rest, tensor)


class _E1Branch(_ParamTree):
    """`encoder.molscribe_encoder` / `encoder.molscribe_projector` (OCSR e1 branch).  The modules are tensor
    containers with the checkpoint's own names and dtypes, so `.state_dict()` / `.parameters()` / save_weights_separately
    (ref: utils/model/utils_model_loading.py:6-46) and `model.safe_load(model.encoder.molscribe_projector, states)`
    (ref: begin.py:151) round-trip them unchanged; the computation - Swin encoder + projector on the HIP engine (e1.E1Engine,
    csrc/swin.hip) - is set up from these tensors when the model is first used (e1_shapes.canonical_*_keys maps timm /
    transformers namings onto the library's).  With an incomplete branch the tokens have to be supplied as `e1=`."""

    def load_state_dict(self, state_dict, strict=False):
        self._modules.clear()
        self._parameters.clear()
        for k, v in state_dict.items():
            self.add(k, torch.as_tensor(v).detach().clone())
        return [], []


class MarkushgrapherForConditionalGeneration(nn.Module):
    main_input_name = "input_ids"

    def __init__(self, config: MarkushgrapherConfig, weight_dtype=torch.bfloat16):
        super().__init__()
        self.config = config
        self._shape = config.to_shape()
        self._weight_dtype = weight_dtype
        self._engine: Optional[Engine] = None
        self._engine_device = None
        self._beam_absorb = (False, 0)      # set_beam_cross_absorb: (on, key splits), applied to every engine / context this model makes
        self._tree = _ParamTree()
        for key, shp, _ in state_dict_spec(self._shape):
            self._tree.add(key, torch.zeros(shp, dtype=weight_dtype))
        self.add_module("encoder", self._tree._modules["encoder"])
        self.add_module("decoder", self._tree._modules["decoder"])
        self.add_module("shared", self._tree._modules["shared"])
        self.add_module("patch_embed", self._tree._modules["patch_embed"])
        self.lm_head = _ParamTree()
        shared_w = self._tree._modules["shared"].weight.data
        self.lm_head.add("weight", shared_w if config.tie_word_embeddings else shared_w.clone())     # tied: stock:1412
        self.encoder.add_module("molscribe_encoder", _E1Branch())
        self.encoder.add_module("molscribe_projector", _E1Branch())
        del self._modules["_tree"]
        self.ignored_keys = []                 # keys of the last load_state_dict that nothing on this path consumes
        self._warned_e1 = False

    # ---- weights ------------------------------------------------------------------------------------------------
    def _canonical_items(self):
        aliases = tied_aliases(self._shape)
        own = dict(super().state_dict())
        for key, _, _ in state_dict_spec(self._shape):
            yield key, own[key]

    def load_state_dict(self, state_dict: Dict[str, torch.Tensor], strict: bool = False):
        aliases = tied_aliases(self._shape)
        own = {k: v for k, v in super().state_dict().items()}
        missing, unexpected = [], []
        seen = set()
        self.ignored_keys = []
        e1_parts = {"encoder.molscribe_encoder.": {}, "encoder.molscribe_projector.": {}}
        for k, v in state_dict.items():
            pref = next((p for p in e1_parts if k.startswith(p)), None)
            if pref is not None:                      # kept on the HF side (round trip), not consumed by the HIP engine
                e1_parts[pref][k[len(pref):]] = v
                continue
            ck = k if k == "lm_head.weight" else aliases.get(k, k)
            if ck in own and ck != "lm_head.weight":
                if tuple(own[ck].shape) != tuple(v.shape):
                    raise ValueError(f"shape mismatch for {k}: {tuple(v.shape)} vs {tuple(own[ck].shape)}")
                own[ck].copy_(torch.as_tensor(v).to(own[ck].dtype))
                seen.add(ck)
            elif k == "lm_head.weight":
                if self.config.tie_word_embeddings:
                    # HF re-ties the head to shared.weight after loading (tie_weights): the checkpoint's tensor is dropped
                    self.lm_head.weight.data = self.shared.weight.data
                    self.ignored_keys.append(k)
                else:
                    self.lm_head.weight.data = torch.as_tensor(v).to(self._weight_dtype).to(self.lm_head.weight.device)
                seen.add(k)
            elif k.startswith("decoder.embed_patches") or k.startswith("decoder.relative_bias"):
                self.ignored_keys.append(k)           # present in UDOP state dicts, never used by the decoder (stock:1212-1213)
            else:
                unexpected.append(k)
        if e1_parts["encoder.molscribe_encoder."]:
            self.encoder.molscribe_encoder.load_state_dict(e1_parts["encoder.molscribe_encoder."])
        if e1_parts["encoder.molscribe_projector."]:
            self.encoder.molscribe_projector.load_state_dict(e1_parts["encoder.molscribe_projector."])
        for key, _, _ in state_dict_spec(self._shape):
            if key not in seen:
                missing.append(key)
        if strict and (missing or unexpected):
            raise RuntimeError(f"missing {missing[:5]}..., unexpected {unexpected[:5]}...")
        self._engine = None     # re-pushed to the HIP arena on next use
        return missing, unexpected

    def safe_load(self, module: nn.Module, state_dict):      # ref: begin.py:151,166
        module.load_state_dict(state_dict, strict=False)
        self._engine = None

    MOLSCRIBE_CKPT = os.path.join("external", "MolScribe", "ckpts", "swin_base_char_aux_1m680k.pth")     # ref: setup.sh:79-82

    def init_molscribe_weights(self, path: Optional[str] = None):
        """ref: begin.py:137-138 - loads the pretrained MolScribe Swin-B (`swin_base_char_aux_1m680k.pth`, ref: setup.sh:79-82) into
        `encoder.molscribe_encoder`.  The checkpoint is looked up at `path`, $MG_MOLSCRIBE_CKPT, or the reference's install location
        relative to the working directory; its `encoder` entry (MolScribe saves {'encoder': ..., 'decoder': ...}, keys possibly behind
        `module.`) is kept under timm's own names.  Without the file the branch keeps what the model checkpoint held (the published
        MarkushGrapher-2 weights carry their frozen copy) and the caller is told."""
        cand = [p for p in (path, os.environ.get("MG_MOLSCRIBE_CKPT"), self.MOLSCRIBE_CKPT) if p]
        hit = next((p for p in cand if os.path.exists(p)), None)
        if hit is None:
            have = len(self.encoder.molscribe_encoder.state_dict())
            warnings.warn(f"markushgrapher_amd: init_molscribe_weights(): no MolScribe checkpoint at {cand}; encoder.molscribe_encoder keeps the "
                          f"{have} tensors of the model checkpoint", stacklevel=2)
            return
        ck = torch.load(hit, map_location="cpu", weights_only=True)
        enc = ck.get("encoder", ck) if isinstance(ck, dict) else ck
        enc = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in enc.items()}
        self.encoder.molscribe_encoder.load_state_dict(enc)
        self._engine = None

    def _e1_setup(self):
        """(E1Shape, canonical state dict) of the OCSR branch when both modules hold a complete set of tensors, else None."""
        from . import e1_shapes
        enc_sd = self.encoder.molscribe_encoder.state_dict()
        prj_sd = self.encoder.molscribe_projector.state_dict()
        if not enc_sd or not prj_sd:
            return None
        import dataclasses
        canon = dict(e1_shapes.canonical_encoder_keys(enc_sd))
        canon.update(e1_shapes.canonical_projector_keys(prj_sd))
        over = {k: (tuple(v) if isinstance(v, list) else v) for k, v in self.config.e1.items()}
        base = dataclasses.replace(e1_shapes.PRESETS["swin_b_384"], d_model=self.config.d_model, src_image_size=self.config.image_size, **over)
        shape = e1_shapes.shape_from_state(base, canon)
        if shape.d_model != self.config.d_model:
            raise ValueError(f"encoder.molscribe_projector ends in {shape.d_model} features, d_model is {self.config.d_model}")
        want = {k: tuple(shp) for k, shp, _ in e1_shapes.state_dict_spec(shape)}
        missing = [k for k in want if k not in canon]
        if missing:
            raise ValueError(f"encoder.molscribe_*: {len(missing)} tensors of the OCSR branch are missing, e.g. {missing[:3]}")
        bad = [k for k in want if tuple(canon[k].shape) != want[k]]
        if bad:
            raise ValueError(f"encoder.molscribe_*: shape mismatch for {bad[:3]} (expected {[want[k] for k in bad[:3]]})")
        return shape, {k: canon[k] for k in want}

    def computes_e1(self) -> bool:
        """True when `encoder.molscribe_encoder` and `encoder.molscribe_projector` hold a complete branch: forward() / generate() then
        evaluate it themselves."""
        return len(self.encoder.molscribe_encoder.state_dict()) > 0 and len(self.encoder.molscribe_projector.state_dict()) > 0

    def requires_e1(self) -> bool:
        """True when the configured architecture fuses the OCSR branch: variant 'me-lf-stack-*' (ref: config/predict.yaml:12,
        utils_model_loading.py:20) or a checkpoint that carries `encoder.molscribe_*` tensors."""
        return str(self.config.architecture_variant).startswith("me-lf-stack") or \
            len(self.encoder.molscribe_encoder.state_dict()) > 0 or len(self.encoder.molscribe_projector.state_dict()) > 0

    def _check_e1(self, e1):
        if e1 is not None or not self.requires_e1():
            return
        if self.computes_e1():
            try:
                self._e1_setup()
            except (KeyError, ValueError) as err:
                raise RuntimeError(f"the encoder.molscribe_* tensors do not form a usable OCSR branch (e1): {err}. Load the complete "
                                   "branch or pass the projected embeddings as e1=[B, M, d_model].") from err
            return
        msg = (f"architecture_variant={self.config.architecture_variant!r}: this model fuses the OCSR vision branch (e1), but "
               "encoder.molscribe_encoder / encoder.molscribe_projector hold no weights to compute it from (load a checkpoint that "
               "carries them, or init_molscribe_weights() + safe_load(model.encoder.molscribe_projector, ...)). Alternatively pass "
               "the projected embeddings as e1=[B, M, d_model]; running without them differs from the reference.")
        if self.config.allow_missing_e1 or os.environ.get("MG_ALLOW_MISSING_E1") == "1":
            if not self._warned_e1:
                warnings.warn(msg + " (allow_missing_e1: continuing with the VTL branch only)", stacklevel=3)
                self._warned_e1 = True
            return
        raise RuntimeError(msg + " Set config.allow_missing_e1 = True (or MG_ALLOW_MISSING_E1=1) to run the VTL branch alone.")

    @classmethod
    def from_pretrained(cls, path, config: Optional[MarkushgrapherConfig] = None, **kw):
        config = config or MarkushgrapherConfig.from_pretrained(path)
        model = cls(config)
        sd = {}
        st = os.path.join(path, "model.safetensors")
        if os.path.exists(st):
            from safetensors.torch import load_file
            sd = load_file(st)
        else:
            sd = torch.load(os.path.join(path, "pytorch_model.bin"), map_location="cpu", weights_only=True)
        model.load_state_dict(sd, strict=False)
        return model.eval()

    def save_pretrained(self, path):
        os.makedirs(path, exist_ok=True)
        with open(os.path.join(path, "config.json"), "w") as f:
            json.dump(self.config.to_dict(), f, indent=1)
        from safetensors.torch import save_file
        out = {k: v.contiguous() for k, v in self._canonical_items()}
        if not self.config.tie_word_embeddings:
            out["lm_head.weight"] = self.lm_head.weight.data.contiguous()
        for name in ("molscribe_encoder", "molscribe_projector"):          # the e1 branch's tensors travel with the checkpoint
            for k, v in getattr(self.encoder, name).state_dict().items():
                out[f"encoder.{name}.{k}"] = v.contiguous()
        save_file(out, os.path.join(path, "model.safetensors"))

    # ---- engine -------------------------------------------------------------------------------------------------
    @property
    def device(self):
        return self.shared.weight.device

    def get_encoder(self):
        return self.encoder

    def _eng(self) -> Engine:
        dev = self.device
        if dev.type != "cuda":
            raise RuntimeError("MarkushgrapherForConditionalGeneration runs on an MI355X only: call .to('cuda') first "
                               "(there is no CPU fallback)")
        if self._engine is None or self._engine_device != dev:
            tied = bool(self.config.tie_word_embeddings)
            eng = Engine(self._shape, mem=TorchMem(dev), max_decode_len=max(512, int(self.config.max_length)),
                         tie_word_embeddings=tied)
            sd = {k: v.data for k, v in self._canonical_items()}
            if not tied:                        # untied config: the checkpoint's head is used, without the d_model^-0.5 scale
                sd["lm_head.weight"] = self.lm_head.weight.data
            eng.load_state_dict(sd)
            if self.computes_e1():              # the OCSR branch on the HIP engine, attached: calls without e1= evaluate it themselves
                from .e1 import E1Engine
                try:
                    shape1, sd1 = self._e1_setup()
                    e1e = E1Engine(shape1, mem=TorchMem(dev)).load_state_dict({k: v.data for k, v in sd1.items()})
                    eng.attach_e1(e1e)
                except (KeyError, ValueError, MgError) as exc:
                    # an incomplete / unsupported branch: the engine stays unattached, so that a caller-supplied e1= still works
                    # (a call WITHOUT e1= then fails in _check_e1 with the reason)
                    self._e1_attach_error = str(exc)
                    warnings.warn(f"OCSR branch (encoder.molscribe_*) not attached to the HIP engine: {exc}; pass e1= explicitly", stacklevel=2)
                else:
                    # What the fork does AROUND the Swin encoder is not in the reference tree (its transformers fork is absent): say once which
                    # choices this build made, so that outputs differing from the reference's are not silent.
                    warnings.warn(
                        "OCSR vision branch attached from the checkpoint's encoder.molscribe_* tensors.  The Swin encoder is pinned on stock "
                        "transformers SwinModel; the steps around it are INFERRED from the reference's README (fork source absent) and unpinned: "
                        f"input = bilinear resize of pixel_values {shape1.src_image_size} -> {shape1.image_size} px with per-channel affine "
                        f"scale {tuple(shape1.pix_scale)} / shift {tuple(shape1.pix_shift)} (MolScribe itself trains on ImageNet mean/std: set "
                        "config.e1 = dict(markushgrapher_amd.e1_shapes.IMAGENET_RENORM) if your checkpoint expects that), projector activation "
                        f"'{shape1.proj_act}', decoder keys = [e1 | VTL states].  Pass e1= to supply the tokens yourself.", stacklevel=2)
            if self._beam_absorb[0]:
                eng.set_beam_cross_absorb(*self._beam_absorb)
            self._engine, self._engine_device = eng, dev
        return self._engine

    def set_beam_cross_absorb(self, on: bool, key_splits: int = 0) -> bool:
        """Beam search (generate(num_beams > 1), generate_queue(num_beams > 1)) with the weight-absorbed cross-attention (Engine.
        set_beam_cross_absorb; default off: the K / V form).  Contexts made afterwards by in_flight() and generate_queue(contexts=...) inherit
        it, as do the ones generate_queue keeps.  Not part of the saved config.  Returns the previous setting."""
        eng = self._eng()
        prev = eng.set_beam_cross_absorb(on, key_splits)
        self._beam_absorb = (bool(on), int(key_splits))
        fl = getattr(self, "_inflight", None)
        if fl is not None:
            for c in fl.contexts:
                if c is not eng:
                    c.set_beam_cross_absorb(on, key_splits)
        return prev

    def _shift_right(self, labels):                          # stock:791-811
        out = labels.new_zeros(labels.shape)
        out[..., 1:] = labels[..., :-1].clone()
        out[..., 0] = self.config.decoder_start_token_id
        out.masked_fill_(out == -100, self.config.pad_token_id)
        return out

    @torch.no_grad()
    def forward(self, input_ids=None, bbox=None, attention_mask=None, pixel_values=None, labels=None,
                decoder_input_ids=None, decoder_attention_mask=None, e1=None, **kw):
        """stock:1448-1574.  Returns logits [B,T,V] fp32 (+ CE loss when labels are given).  e1: optional [B, M, d_model]
        embeddings of the OCSR vision branch (see _E1Branch)."""
        self._check_e1(e1)
        eng = self._eng()
        if decoder_input_ids is None:
            if labels is None:
                raise ValueError("forward() needs labels or decoder_input_ids")
            decoder_input_ids = self._shift_right(labels)
        logits, enc, mask = eng.forward_logits(input_ids, bbox, attention_mask, pixel_values, decoder_input_ids,
                                               decoder_attention_mask, e1=e1)
        loss = None
        if labels is not None:
            loss = nn.functional.cross_entropy(logits.view(-1, logits.size(-1)), labels.to(logits.device).view(-1),
                                               ignore_index=-100)
        return Seq2SeqLMOutput(loss=loss, logits=logits, encoder_last_hidden_state=enc, encoder_attention_mask=mask)

    @torch.no_grad()
    def score(self, input_ids, bbox, pixel_values, attention_mask=None, labels=None, decoder_input_ids=None, e1=None):
        """Log-probability of given target sequences under the model, and the model's own prediction at every position - what the
        reference's evaluation (core/trainers/curriculumTrainer.py:654-672: argmax of the logits against the labels), a loss, or the
        re-ranking of candidates (an n-best list, samples, another OCSR tool's outputs) need - without the [B, T, vocab] logits:
        Engine.score runs the lm_head with the log-softmax, argmax and gather in its epilogue.
        labels [B, T], or [B, C, T] for C candidates per image (one encoder pass, C decoder passes); -100 marks ignored positions, exactly
        as in forward()'s loss; decoder_input_ids default to _shift_right(labels).  -> ScoreOutput.  forward() is unchanged."""
        if labels is None:
            raise ValueError("score() needs labels")
        self._check_e1(e1)
        eng = self._eng()
        if decoder_input_ids is None:
            decoder_input_ids = self._shift_right(labels)
        if tuple(decoder_input_ids.shape) != tuple(labels.shape):
            raise ValueError("decoder_input_ids and labels must have the same shape")
        if labels.dim() == 3:
            tok, arg, alp = eng.score_candidates(input_ids, bbox, attention_mask, pixel_values, decoder_input_ids, labels, e1=e1)
        elif labels.dim() == 2:
            tok, arg, alp = eng.score(input_ids, bbox, attention_mask, pixel_values, decoder_input_ids, labels, e1=e1)
        else:
            raise ValueError(f"labels must be [B, T] or [B, C, T], got {tuple(labels.shape)}")
        live = labels.to(tok.device) != -100
        n = live.sum()
        # (ignored positions hold 0.0: the plain sum is the masked sum; float64: the mean over B * T terms of one call)
        loss = (-(tok.double().sum()) / n.clamp(min=1).double()).float()
        if int(n) == 0:
            loss = loss * float("nan")                  # cross_entropy's mean over no position
        return ScoreOutput(token_logprobs=tok, sequence_logprobs=tok.sum(-1), loss=loss, argmax_ids=arg, argmax_logprobs=alp)

    @torch.no_grad()
    def attribute(self, input_ids, bbox, pixel_values, attention_mask=None, sequences=None, labels=None, decoder_input_ids=None, layers=None,
                  e1=None):
        """Where in the page each token of given sequences came from: the decoder's cross-attention under teacher forcing, averaged over
        heads and the decoder layers `layers` (None: all; an int: that layer; (first, last): inclusive range) - what the reference's
        `config.output_attentions = True` (core/common/begin.py:121) is for, reduced on the device (Engine.attribute) instead of stored
        per layer and head.  Give exactly one of
          sequences  what generate() returned: [B, T + 1] (or [B, C, T + 1]: n-best lists, samples) = start token, tokens, EOS, padding.
                     Decoder inputs are sequences[..., :-1]; row t explains sequences[..., t + 1]; rows after a sequence's first EOS are
                     invalid (a sequence without EOS is valid throughout)
          labels     score()'s convention: [B, T] or [B, C, T], -100 = ignored (invalid row); decoder inputs default to _shift_right(labels)
        -> AttributionOutput.  One encoder pass, one decoder pass per candidate.  generate() and forward() are unchanged.
        Not built: maps from inside generate() / the queue forms, self-attention and encoder maps, per-head or per-layer outputs, rollout or
        gradient-based attribution, the ChemicalOCR stage."""
        if (sequences is None) == (labels is None):
            raise ValueError("attribute() needs exactly one of sequences= and labels=")
        nl = int(self.config.num_decoder_layers)
        if layers is not None:
            rng = (layers, layers) if isinstance(layers, int) else tuple(layers)
            if len(rng) != 2 or not all(isinstance(v, int) for v in rng) or not 0 <= rng[0] <= rng[1] < nl:
                raise ValueError(f"layers must be None, a layer index or (first, last) with 0 <= first <= last < {nl}, got {layers!r}")
            layers = rng
        self._check_e1(e1)
        eng = self._eng()
        dmask = None
        if sequences is not None:
            if decoder_input_ids is not None:
                raise ValueError("decoder_input_ids goes with labels=; sequences= carries its own decoder inputs")
            if sequences.dim() not in (2, 3) or sequences.shape[-1] < 2:
                raise ValueError(f"sequences must be [B, T + 1] or [B, C, T + 1] with T >= 1, got {tuple(sequences.shape)}")
            dec, out_tok = sequences[..., :-1], sequences[..., 1:]
            ended = (out_tok == self.config.eos_token_id).long().cumsum(-1)
            valid = (ended - (out_tok == self.config.eos_token_id).long()) == 0      # up to and including the first EOS
            dmask = valid.to(torch.uint8)
        else:
            if labels.dim() not in (2, 3):
                raise ValueError(f"labels must be [B, T] or [B, C, T], got {tuple(labels.shape)}")
            dec = self._shift_right(labels) if decoder_input_ids is None else decoder_input_ids
            if tuple(dec.shape) != tuple(labels.shape):
                raise ValueError("decoder_input_ids and labels must have the same shape")
            valid = labels != -100
        dec = dec.contiguous()
        if dec.dim() == 3:
            amap, enc_mask = eng.attribute_candidates(input_ids, bbox, attention_mask, pixel_values, dec,
                                                      None if dmask is None else dmask.contiguous(), layers=layers, e1=e1)
        else:
            amap, enc_mask = eng.attribute(input_ids, bbox, attention_mask, pixel_values, dec, dmask, layers=layers, e1=e1)
        if isinstance(amap, np.ndarray):                    # (an engine over a host backend hands back arrays)
            amap = torch.from_numpy(amap)
        valid = valid.to(amap.device)
        if dmask is None:                                  # labels: every position is a decoder position, as in forward(); ignored rows -> 0
            amap = amap * valid[..., None].to(amap.dtype)
        B, L = int(input_ids.shape[0]), int(input_ids.shape[1])
        g = int(self.config.image_size) // int(self.config.patch_size)
        M = int(amap.shape[-1]) - L - g * g
        text, vis = amap[..., M:M + L], amap[..., M + L:]
        pts, recv, keep = patch_assignment(bbox.to(amap.device), attention_mask, g)
        image = pool_to_image(text.reshape(B, -1, L), vis.reshape(B, -1, g * g), pts, recv, keep, g).view(*amap.shape[:-1], g, g)
        return AttributionOutput(cross_attention=amap, valid=valid, e1=amap[..., :M] if M > 0 else None, text=text, image=image)

    def _default_mask(self, input_ids, attention_mask):
        if attention_mask is not None:
            return attention_mask
        pad, eos = self.config.pad_token_id, self.config.eos_token_id
        if pad is not None and pad != eos and bool((input_ids == pad).any()):
            return (input_ids != pad).long()
        return torch.ones_like(input_ids)

    def _sampling_options(self, num_beams, num_return, temperature, top_k, top_p, seed):
        """Defaults and validation of do_sample=True, shared by generate() and generate_queue() -> (temperature, top_k, top_p, seed)."""
        if num_beams > 1:
            raise ValueError("`do_sample=True` with `num_beams` > 1 (beam-sample) is not built; use num_return_sequences for several samples.")
        temperature = 1.0 if temperature is None else float(temperature)
        if top_k is None:
            top_k = getattr(getattr(self, "generation_config", None), "top_k", None)
            top_k = 50 if top_k is None else top_k
        top_p = 1.0 if top_p is None else float(top_p)
        if not temperature > 0.0:
            raise ValueError(f"`temperature` has to be a strictly positive float, got {temperature}")
        if int(top_k) < 0:
            raise ValueError(f"`top_k` has to be a non-negative integer (0 = off), got {top_k}")
        if not 0.0 < top_p <= 1.0:
            raise ValueError(f"`top_p` has to be a float > 0 and <= 1, got {top_p}")
        if num_return < 1:
            raise ValueError(f"`num_return_sequences` has to be >= 1, got {num_return}")
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
        return temperature, int(top_k), top_p, int(seed)

    def _decoder_prompt(self, kw, B, max_length, min_length):
        """The decoder-prompt keywords of generate(), as stock treats them -> (prompt [B, P] int64 or None, lengths [B] int32 numpy or None,
        P of an equal-length prompt (1 without one, None when ragged), max_length, min_length).
          decoder_input_ids [B, P]: stock's start-token rule (_prepare_decoder_input_ids_for_generation) - if NO row starts with
            decoder_start_token_id it is prepended (and a column of ones to the mask).
          decoder_attention_mask [B, P]: the rows' lengths.  UDOP's pad id equals its start id, so padding cannot be read off the values;
            each row must be a run of ones from column 0.  No mask: every row uses the full width.
          max_new_tokens / min_new_tokens: max_length = P + max_new_tokens, min_length = P + min_new_tokens (min_new_tokens wins over
            min_length, as in stock); per-row limits are not built, so ragged prompts refuse them."""
        dec = kw.pop("decoder_input_ids", None)
        dmask = kw.pop("decoder_attention_mask", None)
        max_new, min_new = kw.pop("max_new_tokens", None), kw.pop("min_new_tokens", None)
        lens, P = None, 1
        if dec is None:
            if dmask is not None:
                raise ValueError("`decoder_attention_mask` needs `decoder_input_ids`")
        else:
            dec = torch.as_tensor(dec).to(torch.int64)
            if dec.dim() != 2 or int(dec.shape[0]) != B or int(dec.shape[1]) < 1:
                raise ValueError(f"`decoder_input_ids` must be [{B}, P >= 1], got {tuple(dec.shape)}")
            if dmask is not None:
                dmask = torch.as_tensor(dmask).to(dec.device)
                if tuple(dmask.shape) != tuple(dec.shape):
                    raise ValueError(f"`decoder_attention_mask` must have the shape of `decoder_input_ids` {tuple(dec.shape)}, got {tuple(dmask.shape)}")
                dmask = (dmask != 0).to(torch.int64)
            start = int(self.config.decoder_start_token_id)
            if bool((dec[:, 0] != start).all()):
                dec = torch.cat([torch.full_like(dec[:, :1], start), dec], dim=-1)
                if dmask is not None:
                    dmask = torch.cat([torch.ones_like(dmask[:, :1]), dmask], dim=-1)
            P = int(dec.shape[1])
            if dmask is not None:
                n = dmask.sum(-1)
                run = (torch.arange(P, device=dmask.device)[None, :] < n[:, None]).to(torch.int64)
                if bool((n < 1).any()) or not bool((dmask == run).all()):
                    raise ValueError("every row of `decoder_attention_mask` must be a run of ones from column 0 (the prompt's length); "
                                     "left padding and holes are not supported")
                lens = n.cpu().numpy().astype(np.int32)
                if bool((lens == lens[0]).all()):      # equal lengths: the common width is the prompt
                    P = int(lens[0])
                    dec, lens = dec[:, :P].contiguous(), None
                else:
                    P = None
        if (max_new is not None or min_new is not None) and P is None:
            raise ValueError("`max_new_tokens` / `min_new_tokens` with prompts of different lengths need per-row limits, which are not built; "
                             "pass `max_length` / `min_length`")
        if max_new is not None:
            max_length = P + int(max_new)
        if min_new is not None:
            min_length = P + int(min_new)
        max_length = int(max_length or self.config.max_length)
        if dec is not None:
            longest = int(dec.shape[1]) if lens is None else int(lens.max())
            if longest >= max_length:
                raise ValueError(f"the decoder prompt has {longest} tokens but `max_length` is {max_length}: nothing would be generated; "
                                 "raise `max_length` or pass `max_new_tokens`")
        return dec, lens, P, max_length, int(min_length)

    _CONSTRAINT_KEYS = ("constraint", "suppress_tokens", "begin_suppress_tokens", "bad_words_ids", "prefix_allowed_tokens_fn",
                        "repetition_penalty", "no_repeat_ngram_size")

    @staticmethod
    def _refuse_not_built(kw):
        """the knobs of this family that are not masks, and the callback that cannot run under the captured step: refused, never dropped"""
        if kw.pop("prefix_allowed_tokens_fn", None) is not None:
            raise ValueError("`prefix_allowed_tokens_fn` is a Python callback and cannot run under the captured decode step; compile the rule "
                             "to a token automaton and pass `constraint=` (markushgrapher_amd.constraint)")
        rp = kw.pop("repetition_penalty", None)
        if rp is not None and float(rp) != 1.0:
            raise ValueError(f"`repetition_penalty` is not built (it changes logit values; got {rp}): only 1.0 is accepted")
        ng = kw.pop("no_repeat_ngram_size", None)
        if ng is not None and int(ng) > 0:
            raise ValueError(f"`no_repeat_ngram_size` is not built (it needs unbounded history; got {ng}): only 0 is accepted")

    def _constraint(self, kw, dec, dec_len, B):
        """constraint= (a TokenAutomaton), suppress_tokens=, begin_suppress_tokens=, bad_words_ids= -> (automaton or None, start states [B]).
        All given ones are combined into one product automaton.  With a decoder prompt, image b starts in the state its prompt leaves
        (TokenAutomaton.run_forced over prompt[1:len]: a banned token inside a prompt is accepted, as in stock, and only moves the state);
        begin_suppress_tokens applies at the first free column, so its component starts after the prompt.
        constraint_starts= [B]: image b's state of the USER automaton before its prompt (default 0: one automaton may hold a trie per
        image, constraint.one_of_each)."""
        from . import constraint as K
        self._refuse_not_built(kw)
        user, sup = kw.pop("constraint", None), kw.pop("suppress_tokens", None)
        ustarts = kw.pop("constraint_starts", None)
        if ustarts is not None:
            if user is None:
                raise ValueError("`constraint_starts` needs `constraint`")
            if hasattr(ustarts, "detach"):
                ustarts = ustarts.detach().cpu().numpy()
            ustarts = [int(x) for x in np.asarray(ustarts).reshape(-1)]
            if len(ustarts) != B:
                raise ValueError(f"`constraint_starts` must hold {B} states, got {len(ustarts)}")
        beg, bad = kw.pop("begin_suppress_tokens", None), kw.pop("bad_words_ids", None)
        V, eos = int(self.config.vocab_size), int(self.config.eos_token_id)
        comps = []                                               # (automaton, it follows the prompt)
        if user is not None:
            if not isinstance(user, K.TokenAutomaton):
                raise ValueError("`constraint` must be a markushgrapher_amd.constraint.TokenAutomaton")
            if user.vocab != V or user.eos != eos:
                raise ValueError(f"`constraint` is over {user.vocab} tokens with EOS {user.eos}; the model has {V} and {eos}")
            if ustarts is not None and (min(ustarts) < 0 or max(ustarts) >= user.n_states):
                raise ValueError(f"`constraint_starts` holds a state outside [0, {user.n_states})")
            comps.append((user, True))
        if sup is not None and len(sup):
            comps.append((K.suppress(V, eos, sup), True))
        if bad is not None and len(bad):
            comps.append((K.bad_words(V, eos, bad), True))
        if beg is not None and len(beg):
            comps.append((K.begin_suppress(V, eos, beg), False))
        if not comps:
            return None, None
        rows = [[] for _ in range(B)]
        if dec is not None:
            host = dec.detach().cpu().numpy()
            rows = [host[b, 1:(host.shape[1] if dec_len is None else int(dec_len[b]))] for b in range(B)]
        states = [tuple(a.run_forced(ustarts[b] if (a is user and ustarts is not None) else 0, rows[b]) if follows else 0 for a, follows in comps)
                  for b in range(B)]
        if len(comps) == 1:
            return comps[0][0], np.array([s[0] for s in states], np.int32)
        aut, idx = K.product([a for a, _ in comps], starts=states)
        return aut, np.asarray(idx, np.int32)

    @staticmethod
    def _mask_scores(sc, ids, aut, starts, first, group):
        """output_scores under a constraint: -inf where the row's state does not allow the token, applied on the host from the automaton as
        MinLength is; sc [steps, rows, V] (step t decides column t + 1), row r belongs to image r // group"""
        seq = ids.detach().cpu().numpy() if hasattr(ids, "detach") else np.asarray(ids)
        for r in range(sc.shape[1]):
            st = int(starts[r // group])
            for t in range(first, sc.shape[0]):
                sc[t, r, torch.from_numpy(~aut.allowed_mask(st)).to(sc.device)] = -float("inf")
                st = aut.step(st, seq[r, t + 1])
        return sc

    def _generate_sampled(self, input_ids, bbox, pixel_values, attention_mask, num_beams, max_length, min_length, e1, num_return, as_dict,
                          want_scores, want_logits, kw, prompt=(None, None, 1), con=(None, None)):
        """generate(do_sample=True): stock `_sample` with the temperature / top-k / top-p warpers, drawn on the device
        (include/mgrapher.h mg_generate_sampled).  temperature=1.0, top_k=None (generation_config.top_k if the model has one, else stock's
        default 50; 0 = off), top_p=1.0, num_return_sequences=1, seed=None, stream_ids=None.
        Reproducibility: seed=None draws the call's seed from torch's default CPU generator, so torch.manual_seed(s) makes a sequence of
        calls reproducible and consecutive calls differ; an explicit seed is used as given.  A row's draws depend on (seed, its stream
        id - by default its row index b * num_return_sequences + j - the column) and its own logits only.
        -> [B * num_return_sequences, T], the samples of an image consecutive; return_dict_in_generate: GenerateOutput with token_scores
        (the log-probability of every drawn token under the warped distribution).  output_logits: the raw logits of every step;
        output_scores: those logits after MinLength and temperature (the top-k / top-p filters are applied inside the selection kernel and
        are NOT reflected there).  Both go through the parity capture (eager launches, same ids)."""
        stream_ids = kw.pop("stream_ids", None)
        temperature, top_k, top_p, seed = self._sampling_options(num_beams, num_return, kw.pop("temperature", None), kw.pop("top_k", None),
                                                                 kw.pop("top_p", None), kw.pop("seed", None))
        self._check_e1(e1)
        eng = self._eng()
        max_length = int(max_length or self.config.max_length)
        attention_mask = self._default_mask(input_ids, attention_mask)
        skw = dict(max_length=max_length, min_length=int(min_length), temperature=temperature, top_k=int(top_k), top_p=top_p, seed=int(seed),
                   num_return=num_return, stream_ids=stream_ids, e1=e1, decoder_prompt=prompt[0], decoder_prompt_len=prompt[1],
                   constraint=con[0], constraint_start=con[1])
        first = prompt[2] - 1 if prompt[2] else 0      # output_scores / output_logits hold the free steps only, as stock's do
        if not as_dict:
            return eng.generate_sampled(input_ids, bbox, attention_mask, pixel_values, **skw)[0]
        cap = None
        if want_scores or want_logits:
            cap = eng.debug_decode_capture(max_length - 1, int(input_ids.shape[0]) * num_return)
        try:
            ids, _, ts = eng.generate_sampled(input_ids, bbox, attention_mask, pixel_values, return_scores=True, **skw)
        finally:
            if cap is not None:
                eng.debug_decode_capture()
        out = GenerateOutput(sequences=ids, token_scores=ts)
        if cap is not None:
            steps = int(ids.shape[1]) - 1
            raw = cap[:steps]
            if want_logits:
                out.logits = tuple(raw[t].clone() for t in range(first, steps))
            if want_scores:
                sc = raw.clone()
                for t in range(min(steps, max(0, int(min_length) - 1))):
                    sc[t, :, self.config.eos_token_id] = -float("inf")
                if con[0] is not None:
                    self._mask_scores(sc, ids, con[0], con[1], first, num_return)
                out.scores = tuple(sc[t] / temperature for t in range(first, steps))
        return out

    @torch.no_grad()
    def generate(self, input_ids=None, bbox=None, pixel_values=None, attention_mask=None, labels=None, num_beams=1,
                 max_length=None, min_length=0, length_penalty=1.0, early_stopping=False, do_sample=False, e1=None, **kw):
        """ref call: utils_evaluation.py:269-285 (`labels` arrives as a stray kwarg and is ignored).  Without an
        attention_mask the fork's transformers 4.34 base infers one from pad tokens (all ones at the reference's batch
        size 1), which is what is reproduced here; pass a mask explicitly for padded batches.
        decoder_input_ids= [B, P] (with decoder_attention_mask= for prompts of different lengths): the answers start with the given tokens
        and the model writes the rest, in all three decode modes (include/mgrapher.h mg_generate_prompted; rules: _decoder_prompt).  The
        returned sequences include the prompt, token_scores are 0.0 in its columns, output_scores / output_logits hold the free steps only.
        max_new_tokens= / min_new_tokens= count from the prompt's end (from the start token without one).
        constraint= (a markushgrapher_amd.constraint.TokenAutomaton), suppress_tokens=, begin_suppress_tokens=, bad_words_ids=: constrained
        decoding on the device, greedy and sampled (include/mgrapher.h mg_generate_constrained; rules: _constraint); all given ones are
        combined, in all three decode modes; output_scores holds the masked scores (greedy, sampled; refused for a constrained beam
        search).  constraint_starts= [B]: image b's state of `constraint` before its prompt (default 0; constraint.one_of_each builds one
        automaton with a root per image).  prefix_allowed_tokens_fn= (pass constraint=), repetition_penalty != 1 and no_repeat_ngram_size > 0
        are refused."""
        num_return = int(kw.pop("num_return_sequences", None) or 1)
        as_dict = bool(kw.pop("return_dict_in_generate", False))
        want_scores, want_logits = bool(kw.pop("output_scores", False)), bool(kw.pop("output_logits", False))
        num_beams = int(num_beams)
        dec, dec_len, P, max_length, min_length = self._decoder_prompt(kw, int(input_ids.shape[0]), max_length, min_length)
        if dec is not None and P is None and (want_scores or want_logits):
            raise ValueError("`output_scores` / `output_logits` with prompts of different lengths are not built: the tuples hold one entry "
                             "per free step of the whole batch")
        con, con_start = self._constraint(kw, dec, dec_len, int(input_ids.shape[0]))
        if con is not None and num_beams > 1 and want_scores:
            raise ValueError("`output_scores` of a constrained beam search is not built (the rows' states follow the beams' reordering on the "
                             "device); token_scores and sequences_scores hold the masked values")
        if do_sample:
            return self._generate_sampled(input_ids, bbox, pixel_values, attention_mask, num_beams, max_length, min_length, e1, num_return,
                                          as_dict, want_scores, want_logits, kw, prompt=(dec, dec_len, P), con=(con, con_start))
        if num_beams == 1 and num_return > 1:
            raise ValueError(f"Greedy methods without beam search do not support `num_return_sequences` different than 1 (got {num_return}).")
        if num_return > num_beams:
            raise ValueError("`num_return_sequences` has to be smaller or equal to `num_beams`.")
        self._check_e1(e1)
        eng = self._eng()
        max_length = int(max_length or self.config.max_length)
        attention_mask = self._default_mask(input_ids, attention_mask)
        gkw = dict(num_beams=num_beams, max_length=max_length, min_length=int(min_length), length_penalty=float(length_penalty),
                   early_stopping=early_stopping, e1=e1, decoder_prompt=dec, decoder_prompt_len=dec_len, constraint=con,
                   constraint_start=con_start)
        first = P - 1 if P else 0      # output_scores / output_logits hold the free steps only, as stock's do
        if not as_dict:
            ids, _, _ = eng.generate(input_ids, bbox, attention_mask, pixel_values, num_return=num_return, **gkw)
            return ids
        cap = None
        if want_scores or want_logits:
            # every step's pre-selection logits through the parity instrumentation (eager launches of the same kernels, same ids)
            B = int(input_ids.shape[0])
            cap = eng.debug_decode_capture(max_length - 1, B * num_beams)
        try:
            ids, seq_scores, _, ex = eng.generate(input_ids, bbox, attention_mask, pixel_values, num_return=num_return, return_scores=True,
                                                  **gkw)
        finally:
            if cap is not None:
                eng.debug_decode_capture()
        out = GenerateOutput(sequences=ids, token_scores=ex["token_scores"])
        if num_beams > 1:
            out.sequences_scores, out.beam_indices = seq_scores, ex["beam_indices"].long()
        if cap is not None:
            steps = int(ids.shape[1]) - 1
            raw = cap[:steps]
            if want_logits:
                out.logits = tuple(raw[t].clone() for t in range(first, steps))
            if want_scores:
                # stock's processed scores: log-softmax first for beam search (utils.py:3388-3389), then MinLength (EOS at -inf while
                # the sequence is shorter than min_length)
                sc = torch.log_softmax(raw, dim=-1) if num_beams > 1 else raw.clone()
                eos = self.config.eos_token_id
                for t in range(min(steps, max(0, int(min_length) - 1))):
                    sc[t, :, eos] = -float("inf")
                if con is not None:
                    self._mask_scores(sc, ids, con, con_start, first, 1)
                out.scores = tuple(sc[t] for t in range(first, steps))
        return out

    def compute_transition_scores(self, sequences, scores, beam_indices=None, normalize_logits=False):
        """Stock GenerationMixin.compute_transition_scores (generation/utils.py): the score of every generated token from generate()'s
        `scores` (output_scores=True) -> [rows, generated length].  Greedy: normalize_logits=True gives the token log-probabilities (what
        GenerateOutput.token_scores holds without the full-vocab scores); beam: pass beam_indices, normalize_logits=False."""
        if beam_indices is None:
            beam_indices = torch.arange(scores[0].shape[0], device=sequences.device).view(-1, 1).expand(-1, len(scores))
        V = scores[0].shape[-1]
        stacked = torch.stack(scores).reshape(len(scores), -1).transpose(0, 1)
        if normalize_logits:
            stacked = torch.log_softmax(stacked.reshape(-1, V, stacked.shape[-1]), dim=1).reshape(-1, stacked.shape[-1])
        mask = beam_indices < 0
        max_len = int((1 - mask.long()).sum(-1).max())
        beam_indices = beam_indices.clone()[:, :max_len]
        mask = mask[:, :max_len]
        beam_indices[mask] = 0
        indices = sequences[:, sequences.shape[-1] - max_len:].to(stacked.device) + beam_indices.to(stacked.device) * V
        out = stacked.gather(0, indices)
        out[mask.to(out.device)] = 0
        return out

    @torch.no_grad()
    def in_flight(self, n: int = 4):
        """`inflight.InFlight` over this model's engine: n execution contexts (the engine + n - 1 clones on the same weights), a host
        thread and stream each, for keeping several batches going at once: `with model.in_flight(4) as fl: fl.map(job, batches)`
        where `job(ctx, batch)` calls `ctx.preprocess` / `ctx.generate` (engine level: arrays in, ids out).  DESIGN.md section 8f."""
        from .inflight import InFlight
        self._check_e1(None)
        return InFlight(self._eng(), n)

    def generate_queue(self, encodings, max_length=None, min_length=0, slots=32, chunk=32, contexts=1, num_beams=1, length_penalty=1.0,
                       early_stopping=False, num_return_sequences=1, return_scores=False, do_sample=False, temperature=None, top_k=None,
                       top_p=None, seed=None, **kw):
        """The reference's evaluation loop (ref: utils/ocsr/utils_evaluation.py:140-285) as ONE call: `encodings` = the per-sample
        dicts it builds (input_ids [1, L_n] or [L_n], bbox, pixel_values; attention_mask / labels ignored as there), greedy,
        max_length as there.  Returns a list of 1-D id tensors - predictions[n] == self.generate(**encodings[n], num_beams=1,
        max_length=max_length)[0] - decoded by the continuous decoder (mg_generate_stream: `slots` rows work through the queue, a row
        that emits EOS hands its slot to the next image) with per-image padding semantics (every image computed as if alone).
        contexts > 1: the queue is cut into that many contiguous parts, each decoded by its own execution context (inflight.InFlight,
        at most 4) at the same time - same ids, 1.4 x the images/s at 4.
        num_beams > 1 (the reference's shipped setting, config/predict.yaml beam_search: True -> 5): the beam queue (mg_generate_stream_beam,
        `slots` image slots of num_beams rows, slots * num_beams <= 256); predictions[n] == self.generate(**encodings[n],
        num_beams=num_beams, ...)[0].
        return_scores or num_return_sequences > 1: one dict per image instead - "sequences" [num_return_sequences, T] (the n-best list,
        best first, T = the longest returned hypothesis' columns), "token_scores" [num_return_sequences, T - 1] (as generate()'s
        GenerateOutput.token_scores) and, for beam search, "sequences_scores" [num_return_sequences] and "beam_indices" (numbered as if
        the image were decoded alone).
        do_sample=True: the sampled queue (mg_generate_stream_sampled) - temperature / top_k / top_p / seed with generate(do_sample=True)'s
        defaults and validation, num_beams > 1 refused, num_return_sequences = S samples per image (S * N sequences work through the
        `slots` rows; one encoder pass per image).  predictions[n] == self.generate(**encodings[n], do_sample=True, seed=seed,
        stream_ids=[n * S, ..., n * S + S - 1], num_return_sequences=S, ...) cut at each row's length: sample j of image n draws from
        the random stream n * S + j whatever `slots`, `chunk` and `contexts` are.  S == 1 without return_scores: 1-D id tensors;
        otherwise one dict per image, "sequences" [S, T] (T = the longest sample's columns, shorter ones padded) and "token_scores"
        [S, T - 1] (the log-probability of each drawn token under the warped distribution).
        A decoder prompt per encoding and the constraint options are refused here: generate_queue_constrained() takes them."""
        for k in self._CONSTRAINT_KEYS:      # (constrained decoding belongs to generate(): the queue forms take no constraint)
            if kw.get(k) is not None:
                raise ValueError(f"generate_queue: `{k}` is not supported by the queue forms; constrained decoding is built for generate() only")
        if kw:
            raise TypeError(f"generate_queue() got an unexpected keyword argument '{next(iter(kw))}'")
        for e in encodings:
            if e.get("decoder_input_ids") is not None:
                raise ValueError("generate_queue: an encoding carries `decoder_input_ids`; the queue forms do not take a decoder prompt "
                                 "here (use generate_queue_constrained(), or generate())")
        return self.generate_queue_constrained(encodings, max_length=max_length, min_length=min_length, slots=slots, chunk=chunk, contexts=contexts,
                                               num_beams=num_beams, length_penalty=length_penalty, early_stopping=early_stopping,
                                               num_return_sequences=num_return_sequences, return_scores=return_scores, do_sample=do_sample,
                                               temperature=temperature, top_k=top_k, top_p=top_p, seed=seed)

    def generate_queue_constrained(self, encodings, max_length=None, min_length=0, slots=32, chunk=32, contexts=1, num_beams=1, length_penalty=1.0,
                       early_stopping=False, num_return_sequences=1, return_scores=False, do_sample=False, temperature=None, top_k=None,
                       top_p=None, seed=None, **kw):
        """generate_queue() with a decoder prompt per encoding and the constraint options, in all three modes (the greedy, the sampled and
        the beam queue: mg_generate_stream_constrained / mg_generate_stream_beam_constrained).  Arguments and return values are
        generate_queue()'s; without a prompt and without an option it IS generate_queue().
        constraint= / constraint_starts= [N] / suppress_tokens= / begin_suppress_tokens= / bad_words_ids= as generate() takes them, and an
        encoding may carry `decoder_input_ids` (1-D or [1, P]; lengths may differ across the queue; stock's start-token rule per
        encoding) - predictions[n] == self.generate(**encodings[n], the same options, constraint_starts=[constraint_starts[n]])[0].
        Sequences include the prompt.  Under contexts > 1 every part gets its slice of prompts and start states.
        Refused by name: max_new_tokens / min_new_tokens (per-row limits), output_scores, prefix_allowed_tokens_fn,
        repetition_penalty != 1, no_repeat_ngram_size > 0."""
        from .assembly import collate_for_generate

        def _host_list(x):      # (lengths come back as the engine's memory type: device tensors, or arrays from a host backend)
            return (x.cpu() if hasattr(x, "cpu") else x).tolist()
        for k in ("max_new_tokens", "min_new_tokens"):
            if kw.pop(k, None) is not None:
                raise ValueError(f"generate_queue_constrained: `{k}` needs per-row limits, which are not built; pass `max_length` / `min_length`")
        if kw.pop("output_scores", None):
            raise ValueError("generate_queue_constrained: `output_scores` is not built for the queue forms (return_scores gives the token scores)")
        ckw = {k: kw.pop(k) for k in self._CONSTRAINT_KEYS + ("constraint_starts",) if k in kw}
        if kw:
            raise TypeError(f"generate_queue_constrained() got an unexpected keyword argument '{next(iter(kw))}'")
        num_beams = int(num_beams)
        nr = int(num_return_sequences or 1)
        if do_sample:
            temperature, top_k, top_p, seed = self._sampling_options(num_beams, nr, temperature, top_k, top_p, seed)
        elif num_beams == 1 and nr > 1:
            raise ValueError(f"Greedy methods without beam search do not support `num_return_sequences` different than 1 (got {nr}).")
        if nr > num_beams and not do_sample:
            raise ValueError("`num_return_sequences` has to be smaller or equal to `num_beams`.")
        self._check_e1(None)
        eng = self._eng()
        max_length = int(max_length or self.config.max_length)
        feats, prompts = [], []
        start_id = int(self.config.decoder_start_token_id)
        for e in encodings:
            if e.get("decoder_attention_mask") is not None:
                raise ValueError("generate_queue_constrained: an encoding's `decoder_input_ids` is one prompt of its own length; `decoder_attention_mask` is not taken")
            p = e.get("decoder_input_ids")
            if p is not None:
                p = torch.as_tensor(p).to(torch.int64).cpu()
                if p.dim() == 2 and int(p.shape[0]) == 1:
                    p = p[0]
                if p.dim() != 1 or int(p.shape[0]) < 1:
                    raise ValueError(f"generate_queue_constrained: `decoder_input_ids` of an encoding must be 1-D or [1, P >= 1], got {tuple(p.shape)}")
                if int(p[0]) != start_id:      # stock's start-token rule, for this encoding's batch of one
                    p = torch.cat([torch.tensor([start_id], dtype=torch.int64), p])
                if int(p.shape[0]) >= max_length:
                    raise ValueError(f"the decoder prompt has {int(p.shape[0])} tokens but `max_length` is {max_length}: nothing would be generated")
            prompts.append(p)
            ids = torch.as_tensor(e["input_ids"]).reshape(-1).cpu()
            feats.append({"input_ids": ids, "bbox": torch.as_tensor(e["bbox"]).reshape(-1, 4).cpu().to(torch.float32)})
        batch = collate_for_generate(feats)
        pix = torch.cat([torch.as_tensor(e["pixel_values"]).reshape(1, *torch.as_tensor(e["pixel_values"]).shape[-3:]) for e in encodings]).to(self.device)
        n = len(feats)
        dec = dec_len = None
        if any(p is not None for p in prompts):      # ragged prompts, padded to the longest; an encoding without one holds [start]
            dec_len = np.array([1 if p is None else int(p.shape[0]) for p in prompts], np.int32)
            dec = torch.full((n, int(dec_len.max())), start_id, dtype=torch.int64)
            for i, p in enumerate(prompts):
                if p is not None:
                    dec[i, :dec_len[i]] = p
        con, con_start = self._constraint(ckw, dec, dec_len, n)
        scored = bool(return_scores) or nr > 1
        if num_beams > 1:
            slots = max(1, min(int(slots), 256 // num_beams))
        elif do_sample:
            slots = max(1, min(int(slots), 256))      # the engine's limit of live rows (slots count sequences here)

        def run(ctx, sl):
            m = sl.stop - sl.start
            # every part of the queue gets its slice of the prompts and start states
            pkw = {}
            if dec is not None:
                pkw.update(decoder_prompt=dec[sl], decoder_prompt_len=dec_len[sl])
            if con is not None:
                pkw.update(constraint=con, constraint_start=con_start[sl])
            if do_sample:
                # global stream ids: sequence (part start + i) * S + j, so the result does not depend on `contexts`
                r = ctx.generate_stream_sampled(batch["input_ids"][sl], batch["bbox"][sl], batch["attention_mask"][sl], pix[sl],
                                                max_length=max_length, min_length=int(min_length), temperature=temperature, top_k=top_k,
                                                top_p=top_p, seed=seed, num_return=nr, stream_ids=np.arange(sl.start * nr, sl.stop * nr),
                                                chunk=min(chunk, m), slots=min(slots, m * nr), pool_chunks=3, return_scores=scored, **pkw)
                o, l = r[0], r[1]
            elif num_beams > 1:
                r = ctx.generate_stream_beam(batch["input_ids"][sl], batch["bbox"][sl], batch["attention_mask"][sl], pix[sl],
                                             num_beams=num_beams, max_length=max_length, min_length=int(min_length),
                                             length_penalty=float(length_penalty), early_stopping=bool(early_stopping),
                                             chunk=min(chunk, m), slots=min(slots, m), pool_chunks=3, num_return=nr, return_scores=scored, **pkw)
                o, l = r[0], r[1]
            else:
                r = ctx.generate_stream(batch["input_ids"][sl], batch["bbox"][sl], batch["attention_mask"][sl], pix[sl],
                                        max_length=max_length, min_length=int(min_length), chunk=min(chunk, m), slots=min(slots, m),
                                        pool_chunks=3, return_scores=scored, **pkw)
                o, l = r[0], r[1]
            if scored:
                return o, l, r
            return o, l

        def per_image(o, l, r):
            # o [m * nr, max_length]; the queue's beam indices number the rows of the part's images: renumbered as if each image were alone
            l = _host_list(l)
            res = []
            if do_sample:      # l [m * nr]: every sample has its own length
                for i in range(len(l) // nr):
                    rows = slice(i * nr, (i + 1) * nr)
                    li = max(l[rows])
                    res.append({"sequences": o[rows, :li], "token_scores": r[3][rows, :li - 1]})
                return res
            for i, li in enumerate(l):
                rows = slice(i * nr, (i + 1) * nr)
                d = {"sequences": o[rows, :li]}
                if num_beams > 1:
                    d["sequences_scores"] = r[2][rows]
                    bi = r[4]["beam_indices"][rows, :li - 1].long()
                    d["beam_indices"] = torch.where(bi >= 0, bi - i * num_beams, bi)
                    d["token_scores"] = r[4]["token_scores"][rows, :li - 1]
                else:
                    d["token_scores"] = r[3][i:i + 1, :li - 1]
                res.append(d)
            return res
        contexts = max(1, min(int(contexts), 4, n // max(1, min(slots, n))))
        prev = eng.set_padding_semantics(True)
        try:
            if contexts > 1:
                from .inflight import InFlight
                if getattr(self, "_inflight", None) is None or len(self._inflight) != contexts:
                    if getattr(self, "_inflight", None) is not None:
                        self._inflight.close()
                    self._inflight = InFlight(eng, contexts, include_source=False)      # clones made under per-image padding semantics
                    for c in self._inflight.contexts:
                        c.set_stream_encoder(0)                                         # the contexts overlap one another instead
                per = -(-n // contexts)
                torch.cuda.current_stream(self.device).synchronize()      # the inputs are complete before the contexts' streams read them

                def part(ctx, i):
                    return run(ctx, slice(i * per, min(n, (i + 1) * per)))
                outs = self._inflight.map(part, range(-(-n // per)))
                rows = []
                for res in outs:
                    if scored:
                        rows += per_image(*res)
                        continue
                    o, l = res
                    l = _host_list(l)
                    rows += [o[i, :l[i]] for i in range(len(l))]
                return rows
            res = run(eng, slice(0, n))
        finally:
            eng.set_padding_semantics(prev)
        if scored:
            return per_image(*res)
        ids, lens = res
        lens = _host_list(lens)
        return [ids[i, :lens[i]] for i in range(len(lens))]

