"""Thin ctypes binding of libmgrapher_hip.so (include/mgrapher.h).  PyTorch-ROCm is only the memory carrier:
device buffers are torch tensors, every computation is a HIP kernel behind the C ABI.

`Engine` is written against a tiny memory-provider interface so the parity tests can also drive the SAME C ABI
compiled for the CPU SIMT emulator with numpy buffers (tests/backends.py) — the product default, `TorchMem`, is
the only provider in this package and requires a GPU; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import numpy as np

from . import _lib
from .synth import ModelShape


class MgConfig(C.Structure):
    _fields_ = [(n, C.c_int) for n in (
        "vocab_size", "d_model", "d_kv", "d_ff", "num_layers", "num_decoder_layers", "num_heads",
        "relative_attention_num_buckets", "relative_attention_max_distance", "max_2d_position_embeddings",
        "image_size", "patch_size", "num_channels", "pad_token_id", "eos_token_id", "decoder_start_token_id")] + [
        ("layer_norm_epsilon", C.c_float), ("max_decode_len", C.c_int), ("tie_word_embeddings", C.c_int)]


class MgError(RuntimeError):
    pass


class MgGenOpts(C.Structure):
    """include/mgrapher.h mg_gen_opts: n-best count and the device buffers of the scored generate calls (NULL = not wanted)."""
    _fields_ = [("num_return", C.c_int), ("token_scores", C.c_void_p), ("seq_scores", C.c_void_p), ("beam_indices", C.c_void_p)]


class MgAttrOpts(C.Structure):
    """include/mgrapher.h mg_attr_opts: the inclusive decoder-layer range of mg_decoder_attribute."""
    _fields_ = [("layer_first", C.c_int), ("layer_last", C.c_int)]


class MgSampleOpts(C.Structure):
    """include/mgrapher.h mg_sample_opts: the options of mg_generate_sampled and mg_generate_stream_sampled."""
    _fields_ = [("temperature", C.c_float), ("top_k", C.c_int), ("top_p", C.c_float), ("seed", C.c_uint64), ("stream_ids", C.c_void_p),
                ("num_return", C.c_int), ("token_scores", C.c_void_p)]


class MgDecoderPrompt(C.Structure):
    """include/mgrapher.h mg_decoder_prompt: ids [B][ld] i64 on the device, the lengths [B] i32 on the host."""
    _fields_ = [("ids", C.c_void_p), ("len_host", C.c_void_p), ("ld", C.c_int)]


class MgConstraint(C.Structure):
    """include/mgrapher.h mg_constraint: cls [vocab] u16 and table [n_states][n_classes] i32 on the device, the start states [B] on the host."""
    _fields_ = [("cls", C.c_void_p), ("table", C.c_void_p), ("n_states", C.c_int), ("n_classes", C.c_int), ("start_host", C.c_void_p)]


class MgkConstraint(C.Structure):
    """include/mgrapher.h mgk_constraint (the operator entries mgk_*_constrained): everything on the device, cls padded to the logits' stride."""
    _fields_ = [("cls", C.c_void_p), ("table", C.c_void_p), ("n_states", C.c_int), ("n_classes", C.c_int), ("state", C.c_void_p),
                ("empty", C.c_void_p)]


class TorchMem:
    """Device memory carried by torch tensors on one GPU."""

    def __init__(self, device=None):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("markushgrapher_amd needs an MI355X GPU (torch.cuda.is_available() is False); "
                               "there is no CPU fallback")
        self.torch = torch
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")

    _NP2T = None

    def _dt(self, dtype):
        t = self.torch
        return {np.dtype(np.float32): t.float32, np.dtype(np.float64): t.float64, np.dtype(np.int64): t.int64,
                np.dtype(np.int32): t.int32, np.dtype(np.uint8): t.uint8, np.dtype(np.uint16): t.int16}[np.dtype(dtype)]

    def empty(self, shape, dtype):
        return self.torch.empty(shape, dtype=self._dt(dtype), device=self.device)

    def zeros(self, shape, dtype):
        return self.torch.zeros(shape, dtype=self._dt(dtype), device=self.device)

    def asarray(self, x, dtype):
        """numpy array or torch tensor -> contiguous device tensor of `dtype` (no copy when already right)."""
        t = self.torch
        if isinstance(x, np.ndarray):
            if x.dtype == np.uint16:
                x = x.view(np.int16)
            x = t.from_numpy(np.ascontiguousarray(x))
        want = self._dt(dtype)
        if x.dtype == t.bfloat16 and np.dtype(dtype) == np.uint16:
            x = x.view(t.int16)
        # host sources are copied synchronously: a non-blocking copy from pageable memory may read the (temporary) source after this
        # function has returned and released it (the runtime's queue-thread mode, AMD_DIRECT_DISPATCH=0, does exactly that)
        return x.to(device=self.device, dtype=want, non_blocking=x.is_cuda).contiguous()

    def copy(self, h):
        return h.clone()

    def ptr(self, h):
        return C.c_void_p(h.data_ptr())

    def stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def sync(self):
        # the calling thread's current stream only: a device-wide synchronisation is refused by the runtime ("operation not permitted
        # when stream is capturing") whenever ANOTHER execution context is capturing its decode step at that moment
        self.torch.cuda.current_stream(self.device).synchronize()

    def numpy(self, h):
        self.sync()
        return h.detach().cpu().numpy()


class Engine:
    MAX_LIVE_ROWS = 256     # B * num_beams per generate() call (include/mgrapher.h "Limits")

    def __init__(self, shape: ModelShape, lib=None, mem=None, max_decode_len: int = 512, tie_word_embeddings: bool = True):
        self.lib = lib if lib is not None else _lib.load()
        self.mem = mem if mem is not None else TorchMem()
        self.shape = shape
        self._declare()
        cfg = MgConfig(shape.vocab_size, shape.d_model, shape.d_kv, shape.d_ff, shape.num_layers,
                       shape.num_decoder_layers, shape.num_heads, shape.relative_attention_num_buckets,
                       shape.relative_attention_max_distance, shape.max_2d_position_embeddings, shape.image_size,
                       shape.patch_size, shape.num_channels, shape.pad_token_id, shape.eos_token_id,
                       shape.decoder_start_token_id, shape.layer_norm_epsilon, max_decode_len,
                       1 if tie_word_embeddings else 0)
        self.model = C.c_void_p()
        self._chk(self.lib.mg_create(C.byref(cfg), C.byref(self.model)))
        self.max_decode_len = (max_decode_len + 63) // 64 * 64
        self.arena = self.mem.zeros((int(self.lib.mg_weights_bytes(self.model)),), np.uint8)
        self._chk(self.lib.mg_bind_weights(self.model, self.mem.ptr(self.arena)))
        self._ws = None
        self._ws_bytes = 0
        self._gen_out = {}
        self._samp_out = {}
        self.ignored_keys = []
        self._e1_engine = None

    def _declare(self):
        L = self.lib
        L.mg_last_error.restype = C.c_char_p
        L.mg_weights_bytes.restype = C.c_size_t
        L.mg_weights_bytes.argtypes = [C.c_void_p]
        L.mg_destroy.argtypes = [C.c_void_p]
        L.mg_clone.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.mg_bind_weights.argtypes = [C.c_void_p, C.c_void_p]
        L.mg_finalize.argtypes = [C.c_void_p, C.c_void_p]
        L.mg_load_tensor.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.c_int]
        L.mg_set_decode_graph.argtypes = [C.c_void_p, C.c_int]
        L.mg_attach_e1.argtypes = [C.c_void_p, C.c_void_p]
        L.mg_set_shared_gpu.argtypes = [C.c_void_p, C.c_int]
        L.mg_set_cross_absorb.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.mg_set_beam_cross_absorb.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.mg_decode_graph_active.argtypes = [C.c_void_p]
        L.mg_workspace_bytes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]
        L.mg_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.mg_decoder_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                         C.c_int, C.c_int, C.c_void_p]
        L.mg_score_workspace_bytes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]
        L.mg_decoder_score.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mg_attribute_workspace_bytes.argtypes = L.mg_score_workspace_bytes.argtypes
        L.mg_decoder_attribute.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                           C.POINTER(MgAttrOpts), C.c_void_p]
        L.mg_generate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int,
                                  C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_void_p]
        L.mg_generate_scored.argtypes = L.mg_generate.argtypes + [C.POINTER(MgGenOpts)]
        L.mg_sampled_workspace_bytes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]
        L.mg_generate_sampled.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int), C.c_void_p,
                                          C.POINTER(MgSampleOpts)]
        L.mg_prompted_workspace_bytes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]
        L.mg_generate_prompted.argtypes = L.mg_generate_scored.argtypes + [C.POINTER(MgSampleOpts), C.POINTER(MgDecoderPrompt)]
        L.mg_constrained_workspace_bytes.argtypes = L.mg_prompted_workspace_bytes.argtypes
        L.mg_generate_constrained.argtypes = L.mg_generate_prompted.argtypes + [C.POINTER(MgConstraint)]
        L.mg_stream_workspace_bytes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]
        L.mg_generate_stream.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p] + \
                                        [C.c_int] * 7 + [C.c_void_p, C.c_void_p, C.POINTER(C.c_long)]
        L.mg_stream_beam_workspace_bytes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]
        L.mg_generate_stream_beam.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p] + \
                                             [C.c_int] * 8 + [C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_long)]
        L.mg_generate_stream_scored.argtypes = L.mg_generate_stream.argtypes + [C.POINTER(MgGenOpts)]
        L.mg_generate_stream_sampled.argtypes = L.mg_generate_stream.argtypes + [C.POINTER(MgSampleOpts)]
        L.mg_generate_stream_beam_scored.argtypes = L.mg_generate_stream_beam.argtypes[:-3] + [C.c_void_p, C.POINTER(C.c_long),
                                                                                               C.POINTER(MgGenOpts)]
        L.mg_stream_constrained_workspace_bytes.argtypes = [C.c_void_p] + [C.c_int] * 7 + [C.POINTER(C.c_size_t)]
        L.mg_generate_stream_constrained.argtypes = L.mg_generate_stream_scored.argtypes + [C.POINTER(MgSampleOpts), C.POINTER(MgDecoderPrompt),
                                                                                           C.POINTER(MgConstraint)]
        L.mg_generate_stream_beam_constrained.argtypes = L.mg_generate_stream_beam_scored.argtypes + [C.POINTER(MgDecoderPrompt),
                                                                                                     C.POINTER(MgConstraint)]
        L.mg_stream_encoder_mode.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        L.mg_debug_bucket_table.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int]
        L.mg_debug_decode_capture.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]

    def _chk(self, rc):
        if rc < 0:
            raise MgError(f"libmgrapher error {rc}: {self.lib.mg_last_error().decode()}")
        return rc

    def set_decode_graph(self, mode):
        """0: eager launches; 1: captured decode-step HIP graph (default); 2: the graph's device-counter kernels, eager."""
        return int(self.lib.mg_set_decode_graph(self.model, int(mode)))

    def decode_graph_active(self):
        return bool(self.lib.mg_decode_graph_active(self.model))

    def set_shared_gpu(self, shared: bool) -> bool:
        """Other execution contexts run beside this one (include/mgrapher.h mg_set_shared_gpu): the cross-attention K/V stream keeps one
        workgroup per CU resident so that the other contexts' small launches find wave slots.  InFlight sets it on its contexts.  Returns the
        previous setting."""
        return bool(self.lib.mg_set_shared_gpu(self.model, 1 if shared else 0))

    def set_cross_absorb(self, absorb, key_splits: int = 0):
        """Greedy cross-attention form (include/mgrapher.h mg_set_cross_absorb): True / 1 = weight-absorbed (the layers stream the attended
        encoder states), False / 0 = per-layer K / V streams, "auto" / 2 (default) = by the call's decode rows (absorbed from 96 on).  The
        workspace is re-sized at the next call.  Returns the previous setting (False / True / "auto")."""
        mode = 2 if absorb == "auto" else int(absorb)
        prev = self._chk(self.lib.mg_set_cross_absorb(self.model, mode, int(key_splits)))
        self._ws, self._ws_bytes = None, 0
        return "auto" if prev == 2 else bool(prev)

    @property
    def cross_absorb(self):
        """False / True / "auto": the cross-attention form greedy calls of this context run (mg_set_cross_absorb)."""
        prev = int(self.lib.mg_set_cross_absorb(self.model, -1, 0))
        return "auto" if prev == 2 else bool(prev)

    def set_beam_cross_absorb(self, on: bool, key_splits: int = 0) -> bool:
        """Beam-search cross-attention form (include/mgrapher.h mg_set_beam_cross_absorb), independent of set_cross_absorb: True = weight-
        absorbed (one workgroup serves several beams of an image, every stage of its states read once for all of them), False (default) =
        per-layer K / V streams.  key_splits 1..4 (0 keeps the setting).  Covers generate(num_beams > 1) and generate_stream_beam; clones
        made afterwards inherit it.  The workspaces are re-sized at the next call.  Returns the previous setting."""
        prev = self._chk(self.lib.mg_set_beam_cross_absorb(self.model, 1 if on else 0, int(key_splits)))
        self._ws, self._ws_bytes = None, 0
        self._sws, self._sws_bytes = None, 0
        return bool(prev)

    @property
    def beam_cross_absorb(self) -> bool:
        """True if beam-search calls of this context run the weight-absorbed cross-attention (mg_set_beam_cross_absorb)."""
        return bool(self._chk(self.lib.mg_set_beam_cross_absorb(self.model, -1, 0)))

    ABSORB_AUTO_ROWS = 96      # "auto": calls with at least this many decode rows take the absorbed form (engine.hip MG_ABSORB_AUTO_ROWS)

    def clone(self):
        """A further execution context on this engine's weights (include/mgrapher.h mg_clone): same arena, own workspace, decode
        graph and output buffers.  Calls on different contexts may overlap in time when made from different host threads, each under
        its own stream (`with torch.cuda.stream(s): ctx.generate(...)`); ids per batch are those of a call made alone."""
        other = object.__new__(Engine)
        other.lib, other.mem, other.shape = self.lib, self.mem, self.shape
        other.max_decode_len = self.max_decode_len
        other.arena = self.arena            # shared, kept alive by every context
        other.model = C.c_void_p()
        self._chk(self.lib.mg_clone(self.model, C.byref(other.model)))
        other._ws, other._ws_bytes, other._gen_out, other.ignored_keys = None, 0, {}, list(self.ignored_keys)
        other._samp_out = {}
        other._e1_engine = self._e1_engine      # mg_clone carries the attachment; the branch's weights are shared and kept alive
        return other

    def attach_e1(self, e1_engine):
        """Attach the OCSR vision branch (e1.E1Engine; None detaches): generate() / encode() / the queue forms called without `e1=` then
        evaluate it from pixel_values inside the call and decode over [e1 | e2] (include/mgrapher.h mg_attach_e1) - the reference's
        `architecture_variant: me-lf-stack-1`.  Clones made afterwards inherit it."""
        self.mem.sync()
        self._chk(self.lib.mg_attach_e1(self.model, e1_engine.model if e1_engine is not None else None))
        self._e1_engine = e1_engine
        self._ws, self._ws_bytes, self._gen_out, self._samp_out = None, 0, {}, {}
        self._sws, self._sws_bytes = None, 0
        return self

    def release_workspaces(self):
        """Drop the cached workspaces and output buffers of this context (they are re-allocated by the next call that needs them).  A
        workspace is sized by the largest call the context has seen (14 GB for 64 rows x 512 positions at the large shape): a process
        that moves on to another stage with its own contexts gives the memory back first.  The captured decode graph replays on the
        workspace it was captured on, so the library forgets it as well (mg_set_decode_graph re-arms the capture)."""
        self.mem.sync()
        self._ws, self._ws_bytes, self._gen_out, self._samp_out = None, 0, {}, {}
        self._sws, self._sws_bytes = None, 0
        if self.model:
            prev = self.lib.mg_set_decode_graph(self.model, 0)
            self.lib.mg_set_decode_graph(self.model, prev)

    def close(self):
        if self.model:
            self.lib.mg_destroy(self.model)
            self.model = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------------------------------
    def load_state_dict(self, sd: Dict[str, object], finalize: bool = True):
        """sd: HF state-dict names -> numpy (fp32 / uint16 bf16 bits) or torch tensors (fp32 / bf16)."""
        st = self.mem.stream()
        keep = []
        for key, val in sd.items():
            is_bf16 = (isinstance(val, np.ndarray) and val.dtype == np.uint16) or \
                      (not isinstance(val, np.ndarray) and str(val.dtype) == "torch.bfloat16")
            h = self.mem.asarray(val, np.uint16 if is_bf16 else np.float32)
            keep.append(h)
            shp = (C.c_int64 * len(val.shape))(*[int(s) for s in val.shape])
            rc = self._chk(self.lib.mg_load_tensor(self.model, st, key.encode(), self.mem.ptr(h), 1 if is_bf16 else 0,
                                                   shp, len(val.shape)))
            if rc == 1:
                self.ignored_keys.append(key)
        if finalize:
            self._chk(self.lib.mg_finalize(self.model, st))
        self.mem.sync()
        del keep

    def bucket_table(self, which: int, n: int) -> np.ndarray:
        out = (C.c_int * n)()
        k = self.lib.mg_debug_bucket_table(self.model, which, out, n)
        return np.array(out[:k], dtype=np.int32)

    def workspace(self, B, L, num_beams, max_length, T, M_e1=0, sampled=False, prompted=False, constrained=False):
        """The context's workspace, grown to what the call needs.  sampled: num_beams is the samples per image of a generate_sampled call
        (mg_sampled_workspace_bytes: its rows choose the cross-attention form as greedy rows).  prompted: a call with a decoder prompt
        (mg_prompted_workspace_bytes: the unprompted size plus the prompt lengths).  constrained: a call with a constraint, with or without
        a prompt (mg_constrained_workspace_bytes: the prompted size plus the rows' states, the padded class row and the counter)."""
        need = C.c_size_t()
        if constrained:
            self._chk(self.lib.mg_constrained_workspace_bytes(self.model, B, L, num_beams, max_length, M_e1, 1 if sampled else 0, C.byref(need)))
        elif prompted:
            self._chk(self.lib.mg_prompted_workspace_bytes(self.model, B, L, num_beams, max_length, M_e1, 1 if sampled else 0, C.byref(need)))
        elif sampled:
            self._chk(self.lib.mg_sampled_workspace_bytes(self.model, B, L, num_beams, max_length, M_e1, C.byref(need)))
        else:
            self._chk(self.lib.mg_workspace_bytes(self.model, B, L, num_beams, max_length, T, M_e1, C.byref(need)))
        if need.value > self._ws_bytes:
            self._ws = None
            self._ws = self.mem.empty((need.value,), np.uint8)
            self._ws_bytes = need.value
        return self._ws, self._ws_bytes

    def preprocess(self, pages_u8):
        """u8 pages [B][Hs][Ws][3] (RGB) -> pixel_values [B][3][I][I] f32 on the device: Pillow-LANCZOS resize to the
        model's input size + 1/255 + (x-0.5)/0.5, bit-exact with the reference's host preprocessing
        (ref: core/datasets/mdu_dataset.py:118, core/common/begin.py:105-109)."""
        L = self.lib
        L.mg_preprocess_scratch_bytes.restype = C.c_size_t
        L.mg_preprocess_scratch_bytes.argtypes = [C.c_int] * 4
        L.mg_preprocess_pages.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
        pg = self.mem.asarray(pages_u8, np.uint8)
        B, Hs, Ws, ch = [int(v) for v in pg.shape]
        if ch != self.shape.num_channels:
            raise ValueError("pages must be [B, H, W, 3] uint8")
        I = self.shape.image_size
        nb = int(L.mg_preprocess_scratch_bytes(B, Hs, Ws, I))
        if getattr(self, "_prep_bytes", 0) < nb:
            self._prep = self.mem.empty((nb,), np.uint8)
            self._prep_bytes = nb
        out = self.mem.empty((B, ch, I, I), np.float32)
        self._chk(L.mg_preprocess_pages(self.mem.stream(), self.mem.ptr(pg), B, Hs, Ws, I, self.mem.ptr(out),
                                        self.mem.ptr(self._prep), self._prep_bytes))
        return out

    def _inputs(self, input_ids, bbox, attention_mask, pixel_values):
        ids = self.mem.asarray(input_ids, np.int64)
        bb = self.mem.asarray(bbox, np.float32)
        pv = self.mem.asarray(pixel_values, np.float32)
        am = None if attention_mask is None else self.mem.asarray(attention_mask, np.uint8)
        B, L = int(ids.shape[0]), int(ids.shape[1])
        s = self.shape
        if tuple(bb.shape) != (B, L, 4):
            raise ValueError(f"bbox must be [B,L,4], got {tuple(bb.shape)}")
        if tuple(pv.shape) != (B, s.num_channels, s.image_size, s.image_size):
            raise ValueError(f"pixel_values must be [B,{s.num_channels},{s.image_size},{s.image_size}], got {tuple(pv.shape)}")
        return ids, bb, am, pv, B, L

    def _e1(self, e1, B):
        """e1 [B, M, d_model] fp32: precomputed embeddings of the OCSR vision branch (include/mgrapher.h mg_encode), or None."""
        if e1 is None:
            return None, 0
        t = self.mem.asarray(e1, np.float32)
        if len(t.shape) != 3 or int(t.shape[0]) != B or int(t.shape[2]) != self.shape.d_model or int(t.shape[1]) < 1:
            raise ValueError(f"e1 must be [B, M, {self.shape.d_model}], got {tuple(t.shape)}")
        return t, int(t.shape[1])

    def encode(self, input_ids, bbox, attention_mask, pixel_values, max_length=0, num_beams=1, T=0, want_out=True, e1=None):
        ids, bb, am, pv, B, L = self._inputs(input_ids, bbox, attention_mask, pixel_values)
        e1t, M = self._e1(e1, B)
        ws, nb = self.workspace(B, L, num_beams, max_length, T, M)
        S = L + self.shape.num_patches
        out = self.mem.empty((B, S, self.shape.d_model), np.float32) if want_out else None
        msk = self.mem.empty((B, S), np.uint8) if want_out else None
        self._chk(self.lib.mg_encode(self.model, self.mem.stream(), self.mem.ptr(ws), nb, self.mem.ptr(ids), self.mem.ptr(bb),
                                     self.mem.ptr(am) if am is not None else None, self.mem.ptr(pv),
                                     self.mem.ptr(e1t) if e1t is not None else None, M, B, L,
                                     self.mem.ptr(out) if want_out else None, self.mem.ptr(msk) if want_out else None))
        self._keep = (ids, bb, am, pv, e1t)
        return out, msk

    def forward_logits(self, input_ids, bbox, attention_mask, pixel_values, decoder_input_ids, decoder_attention_mask=None, e1=None):
        dec = self.mem.asarray(decoder_input_ids, np.int64)
        B, T = int(dec.shape[0]), int(dec.shape[1])
        dm = None if decoder_attention_mask is None else self.mem.asarray(decoder_attention_mask, np.uint8)
        enc_out, enc_mask = self.encode(input_ids, bbox, attention_mask, pixel_values, T=T, e1=e1)
        ws, nb = self.workspace(B, int(enc_out.shape[1]) - self.shape.num_patches, 1, 0, T, 0 if e1 is None else int(e1.shape[1]))
        logits = self.mem.empty((B, T, self.shape.vocab_size), np.float32)
        self._chk(self.lib.mg_decoder_forward(self.model, self.mem.stream(), self.mem.ptr(ws), nb, self.mem.ptr(dec),
                                              self.mem.ptr(dm) if dm is not None else None, B, T, self.mem.ptr(logits)))
        return logits, enc_out, enc_mask

    def _score_workspace(self, B, L, T, M_e1):
        """The context's workspace grown to mg_score_workspace_bytes (the teacher-forced layout plus the score kernel's partials).  Called
        BEFORE the encode of a scoring call: a workspace that moved after mg_encode has lost the encoder state."""
        need = C.c_size_t()
        self._chk(self.lib.mg_score_workspace_bytes(self.model, B, L, T, M_e1, C.byref(need)))
        if need.value > self._ws_bytes:
            self._ws = None
            self._ws = self.mem.empty((need.value,), np.uint8)
            self._ws_bytes = need.value
        return self._ws, self._ws_bytes

    def _score_sets(self, enc_args, e1, sets):
        """ONE mg_encode, then one mg_decoder_score per (decoder_input_ids, targets, decoder_attention_mask or None) of `sets`, each [B, T]
        -> [(token_logprobs, argmax_ids, argmax_logprobs)]"""
        sets = [(self.mem.asarray(d, np.int64), self.mem.asarray(t, np.int64), None if m is None else self.mem.asarray(m, np.uint8))
                for d, t, m in sets]
        B, T = (int(v) for v in sets[0][1].shape)
        for d, t, m in sets:
            if len(t.shape) != 2 or any(tuple(x.shape) != (B, T) for x in (d, t, m) if x is not None):
                raise ValueError(f"decoder_input_ids, targets and decoder_attention_mask must all be [{B}, {T}] per candidate")
        if int(enc_args[0].shape[0]) != B:
            raise ValueError(f"targets are for {B} images, the encoder inputs for {int(enc_args[0].shape[0])}")
        L, M_e1 = int(enc_args[0].shape[1]), 0 if e1 is None else int(e1.shape[1])
        ws, nb = self._score_workspace(B, L, T, M_e1)          # (before the encode; Engine.encode's own sizing never shrinks it)
        self.encode(*enc_args, T=T, want_out=False, e1=e1)
        outs = []
        for d, t, m in sets:
            tok, arg, alp = self.mem.empty((B, T), np.float32), self.mem.empty((B, T), np.int64), self.mem.empty((B, T), np.float32)
            self._chk(self.lib.mg_decoder_score(self.model, self.mem.stream(), self.mem.ptr(ws), nb, self.mem.ptr(d),
                                                self.mem.ptr(m) if m is not None else None, self.mem.ptr(t), B, T, self.mem.ptr(tok),
                                                self.mem.ptr(arg), self.mem.ptr(alp)))
            outs.append((tok, arg, alp))
        return outs

    def score(self, input_ids, bbox, attention_mask, pixel_values, decoder_input_ids, targets, decoder_attention_mask=None, e1=None):
        """Log-probabilities of given target tokens under the teacher-forced decoder (mg_decoder_score): the lm_head's log-softmax, argmax
        and gather run in the kernel's epilogue, the [B, T, vocab] logits are never stored.  targets [B, T] int64, a negative target is
        ignored (0.0).  -> token_logprobs [B, T] f32, argmax_ids [B, T] i64, argmax_logprobs [B, T] f32."""
        return self._score_sets((input_ids, bbox, attention_mask, pixel_values), e1, [(decoder_input_ids, targets, decoder_attention_mask)])[0]

    def score_candidates(self, input_ids, bbox, attention_mask, pixel_values, decoder_input_ids, candidates, decoder_attention_mask=None,
                         e1=None):
        """C candidate target sequences per image (an n-best list, samples, another tool's outputs): candidates [B, C, T] int64 with
        decoder_input_ids [B, C, T] (and decoder_attention_mask [B, C, T] or None).  ONE mg_encode, then C mg_decoder_score calls on its
        state.  -> token_logprobs, argmax_ids, argmax_logprobs, each [B, C, T]; candidate c equals score() of it alone, bit for bit."""
        if len(candidates.shape) != 3 or tuple(decoder_input_ids.shape) != tuple(candidates.shape):
            raise ValueError("candidates and decoder_input_ids must both be [B, C, T]")
        dm = decoder_attention_mask
        outs = self._score_sets((input_ids, bbox, attention_mask, pixel_values), e1,
                                [(decoder_input_ids[:, c], candidates[:, c], None if dm is None else dm[:, c]) for c in range(int(candidates.shape[1]))])
        if isinstance(outs[0][0], np.ndarray):
            return tuple(np.stack([o[k] for o in outs], 1) for k in range(3))
        import torch
        return tuple(torch.stack([o[k] for o in outs], 1) for k in range(3))

    def _attr_sets(self, enc_args, e1, sets, layers):
        """ONE mg_encode, then one mg_decoder_attribute per (decoder_input_ids, decoder_attention_mask or None) of `sets`, each [B, T]
        -> ([map [B, T, M_e1 + L + P]], enc_mask [B, L + P])"""
        sets = [(self.mem.asarray(d, np.int64), None if m is None else self.mem.asarray(m, np.uint8)) for d, m in sets]
        if len(sets[0][0].shape) != 2:
            raise ValueError("decoder_input_ids must be [B, T]")
        B, T = (int(v) for v in sets[0][0].shape)
        for d, m in sets:
            if any(tuple(x.shape) != (B, T) for x in (d, m) if x is not None):
                raise ValueError(f"decoder_input_ids and decoder_attention_mask must all be [{B}, {T}] per candidate")
        if int(enc_args[0].shape[0]) != B:
            raise ValueError(f"decoder_input_ids are for {B} images, the encoder inputs for {int(enc_args[0].shape[0])}")
        opts = None
        if layers is not None:
            first, last = (int(layers), int(layers)) if np.isscalar(layers) else (int(layers[0]), int(layers[1]))
            opts = MgAttrOpts(first, last)
        L = int(enc_args[0].shape[1])
        M_e1 = int(e1.shape[1]) if e1 is not None else (self._e1_engine.out_tokens if getattr(self, "_e1_engine", None) is not None else 0)
        need = C.c_size_t()
        self._chk(self.lib.mg_attribute_workspace_bytes(self.model, B, L, T, M_e1, C.byref(need)))
        if need.value > self._ws_bytes:                        # (before the encode: a workspace that moved has lost the encoder state)
            self._ws = None
            self._ws = self.mem.empty((need.value,), np.uint8)
            self._ws_bytes = need.value
        ws, nb = self._ws, self._ws_bytes
        _, enc_mask = self.encode(*enc_args, T=T, e1=e1)
        maps = []
        for d, m in sets:
            out = self.mem.empty((B, T, M_e1 + L + self.shape.num_patches), np.float32)
            self._chk(self.lib.mg_decoder_attribute(self.model, self.mem.stream(), self.mem.ptr(ws), nb, self.mem.ptr(d),
                                                    self.mem.ptr(m) if m is not None else None, B, T,
                                                    C.byref(opts) if opts is not None else None, self.mem.ptr(out)))
            maps.append(out)
        return maps, enc_mask

    def attribute(self, input_ids, bbox, attention_mask, pixel_values, decoder_input_ids, decoder_attention_mask=None, layers=None, e1=None):
        """Where each decoder position looked (mg_decoder_attribute): the teacher-forced cross-attention softmax of the given sequences,
        averaged over heads and the decoder layers `layers` = (first, last) inclusive (an int: that layer; None: all), formed on the chip
        from the cross-attention launch's own Q / K - no [B, H, T, S] tensor exists.  -> map [B, T, M_e1 + L + P] f32 over
        [e1 tokens | text slots | visual slots] and enc_mask [B, L + P] u8.  Unattended keys and rows with decoder_attention_mask == 0 are
        exactly 0; every other row sums to 1."""
        maps, enc_mask = self._attr_sets((input_ids, bbox, attention_mask, pixel_values), e1, [(decoder_input_ids, decoder_attention_mask)], layers)
        return maps[0], enc_mask

    def attribute_candidates(self, input_ids, bbox, attention_mask, pixel_values, decoder_input_ids, decoder_attention_mask=None, layers=None,
                             e1=None):
        """C given sequences per image: decoder_input_ids [B, C, T] (decoder_attention_mask [B, C, T] or None).  ONE mg_encode, then C
        mg_decoder_attribute calls on its state.  -> map [B, C, T, M_e1 + L + P], enc_mask; candidate c equals attribute() of it alone,
        bit for bit."""
        if len(decoder_input_ids.shape) != 3:
            raise ValueError("decoder_input_ids must be [B, C, T]")
        dm = decoder_attention_mask
        maps, enc_mask = self._attr_sets((input_ids, bbox, attention_mask, pixel_values), e1,
                                         [(decoder_input_ids[:, c], None if dm is None else dm[:, c]) for c in range(int(decoder_input_ids.shape[1]))],
                                         layers)
        if isinstance(maps[0], np.ndarray):
            return np.stack(maps, 1), enc_mask
        import torch
        return torch.stack(maps, 1), enc_mask

    def debug_decode_capture(self, capture_steps=0, rows=0, forced_ids=None):
        """Parity-test instrumentation (include/mgrapher.h mg_debug_decode_capture): returns the device buffer
        [capture_steps][rows][vocab] that the next generate() calls fill with their per-step logits; forced_ids
        [B][max_length] teacher-forces the decode path.  Call with no arguments to clear."""
        cap = self.mem.zeros((capture_steps, rows, self.shape.vocab_size), np.float32) if capture_steps > 0 else None
        frc = None if forced_ids is None else self.mem.asarray(forced_ids, np.int64)
        self._dbg_keep = (cap, frc)
        self._chk(self.lib.mg_debug_decode_capture(self.model, self.mem.ptr(cap) if cap is not None else None, capture_steps,
                                                   self.mem.ptr(frc) if frc is not None else None))
        return cap

    def set_padding_semantics(self, per_image: bool):
        """True: every image of a padded batch is computed as if it were alone and unpadded (the reference's batch size is 1);
        False (default): stock HF batched semantics (include/mgrapher.h mg_set_padding_semantics)."""
        self.lib.mg_set_padding_semantics.argtypes = [C.c_void_p, C.c_int]
        return bool(self.lib.mg_set_padding_semantics(self.model, 1 if per_image else 0))

    def set_stream_encoder(self, mode=1, cu_mask=None):
        """Where generate_stream's encoder runs: 0 the caller's stream (serial), 1 its own low-priority stream, 2 its own stream on
        the compute units of `cu_mask` (iterable of CU bit indices)."""
        if mode == 2:
            bits = sorted(set(int(b) for b in cu_mask))
            nw = bits[-1] // 32 + 1
            arr = (C.c_uint32 * nw)()
            for b in bits:
                arr[b // 32] |= 1 << (b % 32)
            self._chk(self.lib.mg_stream_encoder_mode(self.model, 2, arr, nw))
        else:
            self._chk(self.lib.mg_stream_encoder_mode(self.model, int(mode), None, 0))

    def _scored_out(self, key, rows, max_length, beams):
        """Persistent per-shape output buffers of the scored calls (a captured decode step holds their addresses): token scores
        [rows, max_length - 1] and, for beam search, sequence scores [rows] and beam indices [rows, max_length - 1]."""
        cache = self.__dict__.setdefault("_gen_sc", {})
        k = (key, rows, max_length, beams)
        if k not in cache:
            if len(cache) > 8:
                cache.clear()
            cache[k] = (self.mem.zeros((rows, max_length - 1), np.float32),
                        self.mem.zeros((rows,), np.float32) if beams else None,
                        self.mem.zeros((rows, max_length - 1), np.int32) if beams else None)
        ts, ss, bi = cache[k]
        opts = MgGenOpts(1, self.mem.ptr(ts).value, self.mem.ptr(ss).value if ss is not None else None,
                         self.mem.ptr(bi).value if bi is not None else None)
        return opts, ts, ss, bi

    def _prompt(self, decoder_prompt, decoder_prompt_len, B):
        """decoder_prompt [B, P] int64 (+ decoder_prompt_len [B], default all P) -> MgDecoderPrompt, or None without a prompt.  The ids live
        in a buffer kept per (B, P) with the context's persistent buffers: the captured decode step holds its address, so repeated calls
        of one shape replay the step instead of re-capturing it.  Ranges are checked by the library (MG_E_ARG)."""
        if decoder_prompt is None:
            if decoder_prompt_len is not None:
                raise ValueError("decoder_prompt_len needs decoder_prompt")
            return None
        src = self.mem.asarray(decoder_prompt, np.int64)
        if len(src.shape) != 2 or int(src.shape[0]) != B or int(src.shape[1]) < 1:
            raise ValueError(f"decoder_prompt must be [B = {B}, P >= 1], got {tuple(src.shape)}")
        P = int(src.shape[1])
        if decoder_prompt_len is None:
            lens = np.full((B,), P, np.int32)
        else:
            if hasattr(decoder_prompt_len, "detach"):
                decoder_prompt_len = decoder_prompt_len.detach().cpu().numpy()
            lens = np.ascontiguousarray(np.asarray(decoder_prompt_len).reshape(-1).astype(np.int32))
            if lens.shape[0] != B:
                raise ValueError(f"decoder_prompt_len must hold B = {B} lengths, got {lens.shape[0]}")
        cache = self.__dict__.setdefault("_prompt_buf", {})
        if (B, P) not in cache:
            if len(cache) > 8:
                cache.clear()
            cache[(B, P)] = self.mem.zeros((B, P), np.int64)
        buf = cache[(B, P)]
        buf[...] = src
        self._prompt_keep = (buf, lens)
        return MgDecoderPrompt(self.mem.ptr(buf).value, lens.ctypes.data, P)

    def _constraint(self, constraint, constraint_start, B):
        """TokenAutomaton (+ constraint_start [B], default state 0) -> MgConstraint, or None without a constraint.  The tables live in device
        buffers kept per (vocab, states, classes): an automaton is uploaded once, and another one of the same sizes is written IN PLACE, so
        the captured decode step, whose key holds the tables' addresses and sizes, is replayed.  The entries' ranges were checked by
        TokenAutomaton's constructor; the library checks the sizes and the start states (MG_E_ARG)."""
        if constraint is None:
            if constraint_start is not None:
                raise ValueError("constraint_start needs constraint")
            return None
        from .constraint import TokenAutomaton
        if not isinstance(constraint, TokenAutomaton):
            raise TypeError("constraint must be a markushgrapher_amd.constraint.TokenAutomaton")
        if constraint.vocab != self.shape.vocab_size:
            raise ValueError(f"the constraint covers {constraint.vocab} tokens, the model's vocabulary has {self.shape.vocab_size}")
        if constraint_start is None:
            starts = np.zeros((B,), np.int32)
        else:
            if hasattr(constraint_start, "detach"):
                constraint_start = constraint_start.detach().cpu().numpy()
            starts = np.ascontiguousarray(np.asarray(constraint_start).reshape(-1).astype(np.int32))
            if starts.shape[0] != B:
                raise ValueError(f"constraint_start must hold B = {B} states, got {starts.shape[0]}")
        cache = self.__dict__.setdefault("_con_buf", {})
        key = (constraint.vocab, constraint.n_states, constraint.n_classes)
        if key not in cache:
            if len(cache) > 8:
                cache.clear()
            cache[key] = {"cls": self.mem.zeros((key[0],), np.uint16), "table": self.mem.zeros(key[1:], np.int32), "held": None}
        c = cache[key]
        if c["held"] is not constraint:
            c["cls"][...] = self.mem.asarray(constraint.cls, np.uint16)
            c["table"][...] = self.mem.asarray(constraint.table, np.int32)
            c["held"] = constraint
        self._con_keep = (c, starts)
        return MgConstraint(self.mem.ptr(c["cls"]).value, self.mem.ptr(c["table"]).value, key[1], key[2], starts.ctypes.data)

    def generate_sampled(self, input_ids, bbox, attention_mask, pixel_values, max_length=512, min_length=0, temperature=1.0, top_k=0,
                         top_p=1.0, seed=0, num_return=1, stream_ids=None, return_scores=False, return_top2=False, e1=None,
                         decoder_prompt=None, decoder_prompt_len=None, constraint=None, constraint_start=None):
        """Sampled decoding (include/mgrapher.h mg_generate_sampled): temperature, top-k (0 = off), top-p (1 = off) in stock's order, one
        Philox4x32-10 draw per live row and step at counter (stream id, column) under the key `seed`.  -> (ids [B * num_return, cols],
        cols, token_scores [B * num_return, cols - 1] or None[, top2]): row b * num_return + j is sample j of image b.  stream_ids
        [B * num_return] (default: the row index) name the rows' random streams: a row's draws depend on (seed, stream id, column) and its own
        logits only.  decoder_prompt [B, P] / decoder_prompt_len [B]: image b's samples all start with its prompt (mg_generate_prompted);
        forced columns draw nothing and score 0.0.  constraint (a TokenAutomaton) / constraint_start [B] (default state 0): the tokens a
        row's state does not allow leave its distribution before temperature, top-k and top-p (mg_generate_constrained); all samples of
        image b start from constraint_start[b], the state at its first free column (after a prompt: automaton.run(0, prompt[1:len]))."""
        ids, bb, am, pv, B, L = self._inputs(input_ids, bbox, attention_mask, pixel_values)
        nr = int(num_return)
        if nr < 1:
            raise ValueError(f"num_return must be >= 1, got {nr}")
        if not float(temperature) > 0.0:
            raise ValueError(f"temperature must be > 0, got {temperature}")
        if int(top_k) < 0:
            raise ValueError(f"top_k must be >= 0 (0 = off), got {top_k}")
        if not 0.0 < float(top_p) <= 1.0:
            raise ValueError(f"top_p must be in (0, 1], got {top_p}")
        R = B * nr
        if R > self.MAX_LIVE_ROWS:
            raise MgError(f"generate_sampled: B * num_return = {R} live sequences exceeds the supported {self.MAX_LIVE_ROWS}; split the batch")
        e1t, M = self._e1(e1, B)
        prompt = self._prompt(decoder_prompt, decoder_prompt_len, B)
        con = self._constraint(constraint, constraint_start, B)
        ws, nb = self.workspace(B, L, nr, max_length, 0, M, sampled=True, prompted=prompt is not None, constrained=con is not None)
        # persistent output / stream-id buffers: the captured decode step holds their addresses (see generate)
        cache = self._samp_out
        okey = (R, max_length)
        if okey not in cache:
            cache.clear()
            cache[okey] = {"ids": self.mem.empty((R, max_length), np.int64), "ts": self.mem.zeros((R, max_length - 1), np.float32),
                           "sid": None, "sid_host": None}
        c = cache[okey]
        sid = None
        if stream_ids is not None:
            host = np.ascontiguousarray(np.asarray(stream_ids).astype(np.uint64).reshape(-1))
            if host.shape[0] != R:
                raise ValueError(f"stream_ids must hold B * num_return = {R} ids, got {host.shape[0]}")
            if c["sid_host"] is None or not np.array_equal(c["sid_host"], host):
                c["sid"], c["sid_host"] = self.mem.asarray(host.view(np.int64), np.int64), host
            sid = c["sid"]
        top2 = self.mem.zeros((max_length, R, 2), np.float32) if return_top2 else None
        opts = MgSampleOpts(float(temperature), int(top_k), float(top_p), int(seed) & 0xFFFFFFFFFFFFFFFF,
                            self.mem.ptr(sid).value if sid is not None else None, nr,
                            self.mem.ptr(c["ts"]).value if return_scores else None)
        cols = C.c_int(0)
        if con is not None:
            self._chk(self.lib.mg_generate_constrained(
                self.model, self.mem.stream(), self.mem.ptr(ws), nb, self.mem.ptr(ids), self.mem.ptr(bb),
                self.mem.ptr(am) if am is not None else None, self.mem.ptr(pv), self.mem.ptr(e1t) if e1t is not None else None, M, B, L,
                1, max_length, min_length, C.c_float(1.0), 0, self.mem.ptr(c["ids"]), C.byref(cols), None,
                self.mem.ptr(top2) if top2 is not None else None, None, C.byref(opts), C.byref(prompt) if prompt is not None else None,
                C.byref(con)))
        elif prompt is not None:
            self._chk(self.lib.mg_generate_prompted(
                self.model, self.mem.stream(), self.mem.ptr(ws), nb, self.mem.ptr(ids), self.mem.ptr(bb),
                self.mem.ptr(am) if am is not None else None, self.mem.ptr(pv), self.mem.ptr(e1t) if e1t is not None else None, M, B, L,
                1, max_length, min_length, C.c_float(1.0), 0, self.mem.ptr(c["ids"]), C.byref(cols), None,
                self.mem.ptr(top2) if top2 is not None else None, None, C.byref(opts), C.byref(prompt)))
        else:
            self._chk(self.lib.mg_generate_sampled(
                self.model, self.mem.stream(), self.mem.ptr(ws), nb, self.mem.ptr(ids), self.mem.ptr(bb),
                self.mem.ptr(am) if am is not None else None, self.mem.ptr(pv), self.mem.ptr(e1t) if e1t is not None else None, M, B, L,
                max_length, min_length, self.mem.ptr(c["ids"]), C.byref(cols), self.mem.ptr(top2) if top2 is not None else None, C.byref(opts)))
        n = cols.value
        res = (self.mem.copy(c["ids"][:, :n]), n, self.mem.copy(c["ts"][:, :n - 1]) if return_scores else None)
        return res + (top2,) if return_top2 else res

    def _stream_ws(self, chunk, L, slots, pool_chunks, N=0, max_length=0, num_beams=1):
        """The queue's workspace, grown on demand (N > 0: with the extras of a prompted / constrained queue)."""
        need = C.c_size_t()
        if N > 0:
            self._chk(self.lib.mg_stream_constrained_workspace_bytes(self.model, chunk, L, slots, pool_chunks, num_beams, max_length, N,
                                                                     C.byref(need)))
        elif num_beams > 1:
            self._chk(self.lib.mg_stream_beam_workspace_bytes(self.model, chunk, L, slots, pool_chunks, num_beams, max_length, C.byref(need)))
        else:
            self._chk(self.lib.mg_stream_workspace_bytes(self.model, chunk, L, slots, pool_chunks, C.byref(need)))
        if getattr(self, "_sws_bytes", 0) < need.value:
            self._sws = None
            self._sws = self.mem.empty((need.value,), np.uint8)
            self._sws_bytes = need.value

    def _chk_queue(self, rc, outputs):
        """_chk for a prompted / constrained queue call: MG_E_INPUT (an empty allowed set, a prompt id outside the vocabulary) comes after
        the call has completed, so the error carries the outputs (`outputs()` -> what the call would have returned)."""
        try:
            self._chk(rc)
        except MgError as e:
            if rc == -8:
                e.outputs = outputs()
            raise

    def generate_stream(self, input_ids, bbox, attention_mask, pixel_values, max_length=512, min_length=0, chunk=32, slots=32,
                        pool_chunks=3, return_scores=False, decoder_prompt=None, decoder_prompt_len=None, constraint=None,
                        constraint_start=None):
        """Continuous greedy decoding of N images (include/mgrapher.h mg_generate_stream): -> (ids [N, max_length] padded with the pad
        id, lengths [N] = valid columns, decode steps run).  Row n equals generate()'s row for image n.
        return_scores: a fourth item, token_scores [N, max_length - 1] (mg_generate_stream_scored: the log-probability of the token in
        column j + 1 at column j, 0.0 after the image's EOS).
        decoder_prompt [N, P] / decoder_prompt_len [N], constraint (a TokenAutomaton) / constraint_start [N]: per image of the queue, as
        generate() takes them per image of a batch (mg_generate_stream_constrained); row n then equals generate() on image n alone with its
        prompt and start state.  An MgError of code -8 (an empty allowed set, a bad prompt id) carries the completed results in `.outputs`."""
        ids, bb, am, pv, N, L = self._inputs(input_ids, bbox, attention_mask, pixel_values)
        prompt = self._prompt(decoder_prompt, decoder_prompt_len, N)
        con = self._constraint(constraint, constraint_start, N)
        extra = prompt is not None or con is not None
        self._stream_ws(chunk, L, slots, pool_chunks, N if extra else 0, max_length)
        okey = ("stream", N, max_length)
        out = self._gen_out.get(okey)
        if out is None:
            out = self._gen_out[okey] = (self.mem.empty((N, max_length), np.int64), self.mem.empty((N,), np.int32))
        steps = C.c_long(0)
        args = (self.model, self.mem.stream(), self.mem.ptr(self._sws), self._sws_bytes, self.mem.ptr(ids), self.mem.ptr(bb),
                self.mem.ptr(am) if am is not None else None, self.mem.ptr(pv), N, L, chunk, slots, pool_chunks, max_length, min_length,
                self.mem.ptr(out[0]), self.mem.ptr(out[1]), C.byref(steps))
        if not return_scores and not extra:
            self._chk(self.lib.mg_generate_stream(*args))
            return self.mem.copy(out[0]), self.mem.copy(out[1]), int(steps.value)
        opts, ts, _, _ = self._scored_out("stream", N, max_length, False)
        if extra:
            def results():
                res = (self.mem.copy(out[0]), self.mem.copy(out[1]), int(steps.value))
                return res + (self.mem.copy(ts),) if return_scores else res
            self._chk_queue(self.lib.mg_generate_stream_constrained(*args, C.byref(opts) if return_scores else None, None,
                                                                    C.byref(prompt) if prompt is not None else None,
                                                                    C.byref(con) if con is not None else None), results)
            return results()
        self._chk(self.lib.mg_generate_stream_scored(*args, C.byref(opts)))
        return self.mem.copy(out[0]), self.mem.copy(out[1]), int(steps.value), self.mem.copy(ts)

    def generate_stream_sampled(self, input_ids, bbox, attention_mask, pixel_values, max_length=512, min_length=0, temperature=1.0, top_k=0,
                                top_p=1.0, seed=0, num_return=1, stream_ids=None, chunk=32, slots=32, pool_chunks=3, return_scores=False,
                                decoder_prompt=None, decoder_prompt_len=None, constraint=None, constraint_start=None):
        """The greedy queue under sampling (include/mgrapher.h mg_generate_stream_sampled): N images with num_return samples each are a
        queue of N * num_return sequences on `slots` decode rows -> (ids [N * num_return, max_length] padded with the pad id, lengths
        [N * num_return], decode steps run[, token_scores [N * num_return, max_length - 1]]).  Row n * num_return + j is sample j of image
        n and equals generate_sampled() on image n alone with stream id n * num_return + j (stream_ids [N * num_return] names other ids),
        cut at its length.  One encoder pass and one pool entry per image.
        decoder_prompt [N, P] / decoder_prompt_len [N], constraint / constraint_start [N]: per IMAGE, shared by its samples, as
        generate_sampled() takes them (mg_generate_stream_constrained); `.outputs` of an MgError of code -8 as in generate_stream."""
        ids, bb, am, pv, N, L = self._inputs(input_ids, bbox, attention_mask, pixel_values)
        nr = int(num_return)
        if nr < 1:
            raise ValueError(f"num_return must be >= 1, got {nr}")
        if not float(temperature) > 0.0:
            raise ValueError(f"temperature must be > 0, got {temperature}")
        if int(top_k) < 0:
            raise ValueError(f"top_k must be >= 0 (0 = off), got {top_k}")
        if not 0.0 < float(top_p) <= 1.0:
            raise ValueError(f"top_p must be in (0, 1], got {top_p}")
        R = N * nr
        prompt = self._prompt(decoder_prompt, decoder_prompt_len, N)
        con = self._constraint(constraint, constraint_start, N)
        extra = prompt is not None or con is not None
        self._stream_ws(chunk, L, slots, pool_chunks, N if extra else 0, max_length)
        # persistent output / stream-id buffers: the captured decode step holds their addresses
        okey = ("stream-sampled", R, max_length)
        c = self._gen_out.get(okey)
        if c is None:
            c = self._gen_out[okey] = {"ids": self.mem.empty((R, max_length), np.int64), "len": self.mem.empty((R,), np.int32),
                                       "ts": self.mem.zeros((R, max_length - 1), np.float32), "sid": None, "sid_host": None}
        sid = None
        if stream_ids is not None:
            host = np.ascontiguousarray(np.asarray(stream_ids).astype(np.uint64).reshape(-1))
            if host.shape[0] != R:
                raise ValueError(f"stream_ids must hold N * num_return = {R} ids, got {host.shape[0]}")
            if c["sid_host"] is None or not np.array_equal(c["sid_host"], host):
                c["sid"], c["sid_host"] = self.mem.asarray(host.view(np.int64), np.int64), host
            sid = c["sid"]
        opts = MgSampleOpts(float(temperature), int(top_k), float(top_p), int(seed) & 0xFFFFFFFFFFFFFFFF,
                            self.mem.ptr(sid).value if sid is not None else None, nr,
                            self.mem.ptr(c["ts"]).value if return_scores else None)
        steps = C.c_long(0)
        args = (self.model, self.mem.stream(), self.mem.ptr(self._sws), self._sws_bytes, self.mem.ptr(ids), self.mem.ptr(bb),
                self.mem.ptr(am) if am is not None else None, self.mem.ptr(pv), N, L, chunk, slots, pool_chunks, max_length, min_length,
                self.mem.ptr(c["ids"]), self.mem.ptr(c["len"]), C.byref(steps))

        def results():
            res = (self.mem.copy(c["ids"]), self.mem.copy(c["len"]), int(steps.value))
            return res + (self.mem.copy(c["ts"]),) if return_scores else res
        if extra:
            self._chk_queue(self.lib.mg_generate_stream_constrained(*args, None, C.byref(opts), C.byref(prompt) if prompt is not None else None,
                                                                    C.byref(con) if con is not None else None), results)
        else:
            self._chk(self.lib.mg_generate_stream_sampled(*args, C.byref(opts)))
        return results()

    def generate_stream_beam(self, input_ids, bbox, attention_mask, pixel_values, num_beams=5, max_length=512, min_length=0,
                             length_penalty=1.0, early_stopping=False, chunk=32, slots=32, pool_chunks=3, num_return=1, return_scores=False,
                             decoder_prompt=None, decoder_prompt_len=None, constraint=None, constraint_start=None):
        """Continuous BEAM-SEARCH decoding of N images (include/mgrapher.h mg_generate_stream_beam): `slots` image slots of num_beams
        rows -> (ids [N, max_length] = best hypothesis per image, lengths [N], scores [N], decode steps run).  Row n equals
        generate(num_beams=...)'s result for image n.
        num_return > 1: the n-best list - ids [N * num_return, max_length] and scores [N * num_return] (hypotheses of an image consecutive,
        best first), lengths [N] = the longest returned hypothesis' columns.  return_scores: a fifth item, {"token_scores", "beam_indices"}
        [N * num_return, max_length - 1] (mg_generate_stream_beam_scored).
        decoder_prompt [N, P] / decoder_prompt_len [N], constraint / constraint_start [N]: per image of the queue, as generate(num_beams=...)
        takes them per image of a batch (mg_generate_stream_beam_constrained)."""
        ids, bb, am, pv, N, L = self._inputs(input_ids, bbox, attention_mask, pixel_values)
        if slots * num_beams > self.MAX_LIVE_ROWS:
            raise MgError(f"generate_stream_beam: slots * num_beams = {slots * num_beams} rows exceed the supported {self.MAX_LIVE_ROWS}")
        prompt = self._prompt(decoder_prompt, decoder_prompt_len, N)
        con = self._constraint(constraint, constraint_start, N)
        extra = prompt is not None or con is not None
        self._stream_ws(chunk, L, slots, pool_chunks, N if extra else 0, max_length, num_beams)
        nr = int(num_return)
        if not 1 <= nr <= num_beams:
            raise ValueError(f"num_return must be in [1, num_beams = {num_beams}], got {nr}")
        okey = ("stream-beam", N * nr, max_length)
        out = self._gen_out.get(okey)
        if out is None:
            out = self._gen_out[okey] = (self.mem.empty((N * nr, max_length), np.int64), self.mem.empty((N,), np.int32),
                                         self.mem.empty((N * nr,), np.float32))
        steps = C.c_long(0)
        if nr > 1 or return_scores or extra:
            opts, ts, ss, bi = self._scored_out("stream-beam", N * nr, max_length, True)
            opts.num_return = nr
            if not return_scores:
                opts.token_scores = opts.beam_indices = None
            args = (self.model, self.mem.stream(), self.mem.ptr(self._sws), self._sws_bytes, self.mem.ptr(ids), self.mem.ptr(bb),
                    self.mem.ptr(am) if am is not None else None, self.mem.ptr(pv), N, L, chunk, slots, pool_chunks, num_beams, max_length,
                    min_length, C.c_float(length_penalty), 1 if early_stopping else 0, self.mem.ptr(out[0]), self.mem.ptr(out[1]), C.byref(steps),
                    C.byref(opts))
            if extra:
                self._chk(self.lib.mg_generate_stream_beam_constrained(*args, C.byref(prompt) if prompt is not None else None,
                                                                       C.byref(con) if con is not None else None))
                if nr == 1 and not return_scores:
                    return self.mem.copy(out[0]), self.mem.copy(out[1]), self.mem.copy(ss), int(steps.value)
            else:
                self._chk(self.lib.mg_generate_stream_beam_scored(*args))
            res = (self.mem.copy(out[0]), self.mem.copy(out[1]), self.mem.copy(ss), int(steps.value))
            if return_scores:
                res += ({"token_scores": self.mem.copy(ts), "beam_indices": self.mem.copy(bi)},)
            return res
        self._chk(self.lib.mg_generate_stream_beam(self.model, self.mem.stream(), self.mem.ptr(self._sws), self._sws_bytes, self.mem.ptr(ids),
                                                   self.mem.ptr(bb), self.mem.ptr(am) if am is not None else None, self.mem.ptr(pv), N, L, chunk,
                                                   slots, pool_chunks, num_beams, max_length, min_length, C.c_float(length_penalty),
                                                   1 if early_stopping else 0, self.mem.ptr(out[0]), self.mem.ptr(out[1]),
                                                   self.mem.ptr(out[2]), C.byref(steps)))
        return self.mem.copy(out[0]), self.mem.copy(out[1]), self.mem.copy(out[2]), int(steps.value)

    def generate(self, input_ids, bbox, attention_mask, pixel_values, num_beams=1, max_length=512, min_length=0,
                 length_penalty=1.0, early_stopping=False, return_top2=False, e1=None, num_return=1, return_scores=False,
                 decoder_prompt=None, decoder_prompt_len=None, constraint=None, constraint_start=None):
        """-> (ids [B, cols], scores [B] (beam: sequences_scores), top2 or None).  num_return (beam: 1 .. num_beams): the n-best list,
        ids [B * num_return, cols] and scores [B * num_return], hypotheses of an image consecutive, best first; cols = the longest
        returned hypothesis'.  return_scores: a fourth item {"token_scores": [rows, cols - 1], "beam_indices": [rows, cols - 1] (beam) or
        None} - include/mgrapher.h mg_generate_scored.
        decoder_prompt [B, P] int64 / decoder_prompt_len [B] (default all P): image b's rows start with decoder_prompt[b, :len[b]] and
        decode freely from there (include/mgrapher.h mg_generate_prompted); the returned ids include the prompt, token_scores are 0.0 in
        its columns.
        constraint (a TokenAutomaton) / constraint_start [B] (default state 0): greedy decoding under the automaton
        (mg_generate_constrained) - a token the row's state does not allow cannot be chosen and is left out of top2 and of the token
        scores' normaliser; constraint_start[b] is image b's state at its first free column (after a prompt: automaton.run(0,
        prompt[1:len])).  A greedy call runs the unfused selection tail.  Beam search: the mask sets a candidate's log-probability to -inf
        after the log-softmax over the raw logits, as stock's processors do; the K rows' states follow the beams."""
        ids, bb, am, pv, B, L = self._inputs(input_ids, bbox, attention_mask, pixel_values)
        nr = int(num_return)
        if not 1 <= nr <= num_beams:
            raise ValueError(f"num_return must be in [1, num_beams = {num_beams}], got {nr}")
        e1t, M = self._e1(e1, B)
        if B * num_beams > self.MAX_LIVE_ROWS:
            raise MgError(f"generate: B * num_beams = {B * num_beams} live sequences exceeds the supported "
                          f"{self.MAX_LIVE_ROWS}; split the batch")
        prompt = self._prompt(decoder_prompt, decoder_prompt_len, B)
        con = self._constraint(constraint, constraint_start, B)
        ws, nb = self.workspace(B, L, num_beams, max_length, 0, M, prompted=prompt is not None, constrained=con is not None)
        p_ref = C.byref(prompt) if prompt is not None else None
        # the id buffer is persistent per (B, max_length): the captured decode-step graph holds its address, so a stable
        # buffer lets later calls replay the graph instead of re-capturing; callers get a copy
        okey = (B * nr, max_length)
        out = self._gen_out.get(okey)
        if out is None:
            self._gen_out.clear()
            out = self._gen_out[okey] = self.mem.empty((B * nr, max_length), np.int64)
        scores = self.mem.zeros((B * nr,), np.float32)
        top2 = self.mem.zeros((max_length, B * num_beams, 2), np.float32) if (return_top2 and num_beams == 1) else None
        cols = C.c_int(0)
        args = (self.model, self.mem.stream(), self.mem.ptr(ws), nb, self.mem.ptr(ids), self.mem.ptr(bb),
                self.mem.ptr(am) if am is not None else None, self.mem.ptr(pv), self.mem.ptr(e1t) if e1t is not None else None, M, B, L,
                num_beams, max_length, min_length, C.c_float(length_penalty), 1 if early_stopping is True else 0,
                self.mem.ptr(out), C.byref(cols), self.mem.ptr(scores), self.mem.ptr(top2) if top2 is not None else None)
        if nr == 1 and not return_scores:
            if con is not None:
                self._chk(self.lib.mg_generate_constrained(*args, None, None, p_ref, C.byref(con)))
            elif prompt is not None:
                self._chk(self.lib.mg_generate_prompted(*args, None, None, C.byref(prompt)))
            else:
                self._chk(self.lib.mg_generate(*args))
            return self.mem.copy(out[:, :cols.value]), scores, top2
        beam = num_beams > 1
        opts, ts, _, bi = self._scored_out("batch", B * nr, max_length, beam)
        opts.num_return = nr
        opts.seq_scores = self.mem.ptr(scores).value if beam else None
        if not return_scores:
            opts.token_scores = opts.beam_indices = None
        if con is not None:
            self._chk(self.lib.mg_generate_constrained(*args, C.byref(opts), None, p_ref, C.byref(con)))
        elif prompt is not None:
            self._chk(self.lib.mg_generate_prompted(*args, C.byref(opts), None, C.byref(prompt)))
        else:
            self._chk(self.lib.mg_generate_scored(*args, C.byref(opts)))
        n = cols.value
        res = (self.mem.copy(out[:, :n]), scores, top2)
        if return_scores:
            res += ({"token_scores": self.mem.copy(ts[:, :n - 1]), "beam_indices": self.mem.copy(bi[:, :n - 1]) if beam else None},)
        return res
