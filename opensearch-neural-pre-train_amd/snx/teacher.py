"""Dense teacher encoder: the forward of an XLM-RoBERTa encoder with CLS pooling (BGE-M3's dense head) on the GPU
(csrc/teacher.hip, include/snx.h "dense teacher encoder").

    enc = TeacherEncoder.from_pretrained("/models/bge-m3", device="cuda:0", precision="bf16")
    emb = enc.encode(texts, tokenizer, max_length=256)                 # fp32 [n, hidden], unit rows, input order
    emb = enc.encode_tokens(input_ids, attention_mask)                 # the same from a padded batch

``forward_torch`` restates the same forward in plain torch (fp32, no transformers import): it is what a ``TeacherEncoder``
on a ``cpu`` device runs, and the comparator of the GPU tests.  Its ``emulate_bf16`` mode rounds at exactly the cast points
of the bf16 path: GEMM operands and GEMM outputs are bf16 (a bias added to a bf16 GEMM output that feeds another GEMM or
the attention is rounded again; the attention's probabilities enter P V as bf16 in their unnormalised form exp(s - max),
the row sum that divides the product stays fp32), the residual stream and all LayerNorm / GELU / softmax arithmetic stay
fp32.

A model is only ever read from a local directory; a model name is never resolved."""
from __future__ import annotations

import ctypes as C
import json
import os
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from ._abi import CONSTANTS, STRUCTS

PRECISIONS = {"bf16": CONSTANTS["SNX_TEACHER_BF16"], "fp32": CONSTANTS["SNX_TEACHER_F32"]}
DEFAULT_BATCH_TOKENS = 16384           # token rows per forward of ``encode``
TeacherDesc = STRUCTS["snx_teacher_desc"]


@dataclass
class TeacherConfig:
    """The architecture constants of the encoder (field names follow the HF config.json); defaults: BGE-M3."""
    vocab_size: int = 250002
    hidden_size: int = 1024
    intermediate_size: int = 4096
    num_hidden_layers: int = 24
    num_attention_heads: int = 16
    max_position_embeddings: int = 8194
    type_vocab_size: int = 1
    pad_token_id: int = 1
    layer_norm_eps: float = 1e-5

    @property
    def head_dim(self) -> int:
        return self.hidden_size // self.num_attention_heads

    @classmethod
    def from_hf(cls, cfg: dict) -> "TeacherConfig":
        if cfg.get("model_type") != "xlm-roberta":
            raise ValueError(f"teacher: config.json has model_type {cfg.get('model_type')!r}, expected 'xlm-roberta'")
        if cfg.get("hidden_act", "gelu") != "gelu":
            raise ValueError(f"teacher: hidden_act {cfg.get('hidden_act')!r} is not supported (erf GELU only)")
        if cfg.get("position_embedding_type", "absolute") != "absolute":
            raise ValueError("teacher: only absolute position embeddings are supported")
        names = [f for f in cls.__dataclass_fields__]
        return cls(**{k: cfg[k] for k in names if k in cfg})

    def validate(self) -> None:
        H = self.hidden_size
        if H <= 0 or H % 256 or H > 1024:
            raise ValueError("teacher: hidden_size must be a multiple of 256, at most 1024")
        if self.num_attention_heads <= 0 or H % self.num_attention_heads or self.head_dim != 64:
            raise ValueError("teacher: head_dim must be 64")
        if self.intermediate_size <= 0 or self.intermediate_size % 64:
            raise ValueError("teacher: intermediate_size must be a multiple of 64")
        if not 1 <= self.num_hidden_layers <= 128:
            raise ValueError("teacher: num_hidden_layers must lie in [1, 128]")
        if self.vocab_size <= 0 or self.max_position_embeddings <= 0 or self.type_vocab_size <= 0 or self.pad_token_id < 0:
            raise ValueError("teacher: vocab_size, max_position_embeddings, type_vocab_size must be positive")

    def desc(self) -> TeacherDesc:
        return TeacherDesc(self.vocab_size, self.hidden_size, self.intermediate_size, self.num_hidden_layers,
                           self.num_attention_heads, self.head_dim, self.max_position_embeddings, self.type_vocab_size,
                           self.pad_token_id, 0, float(self.layer_norm_eps), 0.0)


_LAYER_KEYS = ("attention.self.query", "attention.self.key", "attention.self.value", "attention.output.dense",
               "attention.output.LayerNorm", "intermediate.dense", "output.dense", "output.LayerNorm")


def param_keys(config: TeacherConfig) -> List[str]:
    """State-dict keys (no ``roberta.`` prefix) in the canonical order of the C ABI (include/snx.h)."""
    keys = ["embeddings.word_embeddings.weight", "embeddings.position_embeddings.weight",
            "embeddings.token_type_embeddings.weight", "embeddings.LayerNorm.weight", "embeddings.LayerNorm.bias"]
    for l in range(config.num_hidden_layers):
        for k in _LAYER_KEYS:
            keys += [f"encoder.layer.{l}.{k}.weight", f"encoder.layer.{l}.{k}.bias"]
    return keys


def param_shapes(config: TeacherConfig) -> Dict[str, Tuple[int, ...]]:
    H, I = config.hidden_size, config.intermediate_size
    out = {"embeddings.word_embeddings.weight": (config.vocab_size, H),
           "embeddings.position_embeddings.weight": (config.max_position_embeddings, H),
           "embeddings.token_type_embeddings.weight": (config.type_vocab_size, H),
           "embeddings.LayerNorm.weight": (H,), "embeddings.LayerNorm.bias": (H,)}
    for l in range(config.num_hidden_layers):
        p = f"encoder.layer.{l}."
        for k in _LAYER_KEYS:
            if k.endswith("LayerNorm"):
                w = (H,)
            elif k == "intermediate.dense":
                w = (I, H)
            elif k == "output.dense":
                w = (H, I)
            else:
                w = (H, H)
            out[p + k + ".weight"] = w
            out[p + k + ".bias"] = (w[0],)
    return out


def hf_parameter_order(config: TeacherConfig) -> List[str]:
    """The keys in the order of XLMRobertaModel(add_pooling_layer=False).named_parameters() (its embeddings register
    word, token_type, LayerNorm, position)."""
    keys = param_keys(config)
    return [keys[0], keys[2], keys[3], keys[4], keys[1]] + keys[5:]


def random_state_dict(config: TeacherConfig, seed: int) -> Dict[str, torch.Tensor]:
    """Weights from a recipe instead of a file (goldens, tests, benchmarks): one numpy.random.RandomState(seed), drawn in
    ``hf_parameter_order``; matrices and embeddings N(0, 0.1), biases 0.1 N(0, 1), LayerNorm weights 1 + 0.2 N(0, 1), each
    drawn in float64 and cast to fp32.  (The usual 0.02 initialisation makes all embeddings of a tiny model agree to
    cosine 0.999: a masking or position error would then barely move them.)"""
    import numpy as np
    rs = np.random.RandomState(int(seed))
    shapes = param_shapes(config)
    out = {}
    for k in hf_parameter_order(config):
        z = rs.standard_normal(shapes[k])
        if k.endswith(".bias"):
            v = 0.1 * z
        elif "LayerNorm" in k:
            v = 1.0 + 0.2 * z
        else:
            v = 0.1 * z
        out[k] = torch.from_numpy(v.astype(np.float32))
    return out


def normalize_state_dict(config: TeacherConfig, state_dict: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The encoder's tensors as fp32, keyed without the ``roberta.`` prefix; pooler, LM-head and buffer keys are dropped.
    A missing tensor or a wrong shape raises."""
    sd = {(k[len("roberta."):] if k.startswith("roberta.") else k): v for k, v in state_dict.items()}
    shapes = param_shapes(config)
    out = {}
    for k in param_keys(config):
        if k not in sd:
            raise KeyError(f"teacher: state dict has no {k!r}")
        v = sd[k]
        if tuple(v.shape) != shapes[k]:
            raise ValueError(f"teacher: {k} has shape {tuple(v.shape)}, expected {shapes[k]}")
        out[k] = v.detach().to(torch.float32)
    return out


def position_ids(attention_mask: torch.Tensor, pad_id: int) -> torch.Tensor:
    """XLM-R positions from the mask: cumsum(mask) * mask + pad_id (a right-padded row starts at pad_id + 1)."""
    m = attention_mask.to(torch.long)
    return torch.cumsum(m, dim=1) * m + int(pad_id)


def _check_batch(config: TeacherConfig, input_ids, attention_mask) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    if not isinstance(input_ids, torch.Tensor) or not isinstance(attention_mask, torch.Tensor) or input_ids.dim() != 2 or \
            input_ids.shape != attention_mask.shape or input_ids.is_floating_point() or attention_mask.is_floating_point():
        raise ValueError("teacher: input_ids and attention_mask must be int tensors of one shape [n, S]")
    if input_ids.shape[0] == 0 or input_ids.shape[1] == 0:
        raise ValueError("teacher: empty batch")
    ids, mask = input_ids.to(torch.long), (attention_mask != 0).to(torch.long)
    if bool((mask.sum(dim=1) == 0).any()):
        raise ValueError("teacher: a row of attention_mask is all zero")
    if bool(((ids < 0) | (ids >= config.vocab_size)).any()):
        raise ValueError(f"teacher: input_ids must lie in [0, {config.vocab_size})")
    pos = position_ids(mask, config.pad_token_id)
    if int(pos.max()) >= config.max_position_embeddings:
        raise ValueError(f"teacher: position {int(pos.max())} >= max_position_embeddings {config.max_position_embeddings}")
    return ids, mask, pos


def forward_torch(config: TeacherConfig, params: Dict[str, torch.Tensor], input_ids: torch.Tensor,
                  attention_mask: torch.Tensor, emulate_bf16: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """XLMRobertaModel(add_pooling_layer=False) in eval mode on a padded batch, in plain fp32 torch -> (cls fp32 [n, H] =
    the row of every sequence's first token, emb = F.normalize(cls)).  ``params``: ``normalize_state_dict``'s tensors.
    ``emulate_bf16``: round at the cast points of the GPU's bf16 path (module docstring)."""
    ids, mask, pos = _check_batch(config, input_ids, attention_mask)
    n, S = ids.shape
    H, heads, eps = config.hidden_size, config.num_attention_heads, config.layer_norm_eps
    dev = params["embeddings.LayerNorm.weight"].device
    ids, mask, pos = ids.to(dev), mask.to(dev), pos.to(dev)

    def r(t):
        return t.to(torch.bfloat16).to(torch.float32) if emulate_bf16 else t

    def ln(x, key):
        return F.layer_norm(x, (H,), params[key + ".weight"], params[key + ".bias"], eps)

    e = "embeddings."
    x = (params[e + "word_embeddings.weight"][ids] + params[e + "token_type_embeddings.weight"][0]) + \
        params[e + "position_embeddings.weight"][pos]
    h = ln(x, e + "LayerNorm")
    key_bias = torch.zeros((n, 1, 1, S), dtype=torch.float32, device=dev).masked_fill(mask[:, None, None, :] == 0,
                                                                                         float("-inf"))
    for l in range(config.num_hidden_layers):
        p = f"encoder.layer.{l}."
        xb = r(h)
        wqkv = torch.cat([params[p + f"attention.self.{k}.weight"] for k in ("query", "key", "value")])
        bqkv = torch.cat([params[p + f"attention.self.{k}.bias"] for k in ("query", "key", "value")])
        qkv = r(r(xb @ r(wqkv).t()) + bqkv)
        q, k, v = (t.reshape(n, S, heads, 64).transpose(1, 2) for t in qkv.split(H, dim=-1))
        score = (q @ k.transpose(2, 3)) * 0.125 + key_bias
        prob = torch.exp(score - score.amax(dim=-1, keepdim=True))                   # softmax, normalised after P V:
        a = (r(prob) @ v) / prob.sum(dim=-1, keepdim=True)                           # P is the bf16 operand of that GEMM
        a = r(a.transpose(1, 2).reshape(n, S, H))
        y = r(a @ r(params[p + "attention.output.dense.weight"]).t())
        h = ln((y + params[p + "attention.output.dense.bias"]) + h, p + "attention.output.LayerNorm")
        xb = r(h)
        u = r(xb @ r(params[p + "intermediate.dense.weight"]).t())
        u = r(F.gelu(u + params[p + "intermediate.dense.bias"]))
        y = r(u @ r(params[p + "output.dense.weight"]).t())
        h = ln((y + params[p + "output.dense.bias"]) + h, p + "output.LayerNorm")
    first = mask.argmax(dim=1)
    cls = h[torch.arange(n, device=dev), first]
    return cls, F.normalize(cls, p=2, dim=-1)


def _read_weights(model_dir: str) -> Dict[str, torch.Tensor]:
    st = os.path.join(model_dir, "model.safetensors")
    if os.path.exists(st):
        from safetensors.torch import load_file
        return load_file(st, device="cpu")
    pt = os.path.join(model_dir, "pytorch_model.bin")
    if os.path.exists(pt):
        return torch.load(pt, map_location="cpu", weights_only=True)
    raise FileNotFoundError(f"teacher: {model_dir} holds neither model.safetensors nor pytorch_model.bin")


def _check_pooling(model_dir: str) -> None:
    path = os.path.join(model_dir, "1_Pooling", "config.json")
    if not os.path.exists(path):
        return
    with open(path) as f:
        cfg = json.load(f)
    others = [k for k, v in cfg.items() if k.startswith("pooling_mode_") and k != "pooling_mode_cls_token" and v]
    if not cfg.get("pooling_mode_cls_token", False) or others:
        raise ValueError(f"teacher: {path} does not describe CLS pooling (only pooling_mode_cls_token is supported)")


def _length_batches(lens: Sequence[int], batch_size: Optional[int], batch_tokens: int):
    """The batches of ``TeacherEncoder.encode``: the rows sorted by length (stable: equal lengths keep input order) and cut
    into runs of at most ``batch_tokens`` token rows and ``batch_size`` sequences; a longer single row runs alone."""
    order = sorted(range(len(lens)), key=lambda i: lens[i])
    batch: List[int] = []
    rows = 0
    for i in order:
        if batch and (rows + lens[i] > int(batch_tokens) or (batch_size is not None and len(batch) >= int(batch_size))):
            yield batch
            batch, rows = [], 0
        batch.append(i)
        rows += lens[i]
    if batch:
        yield batch


class TeacherEncoder:
    """The dense teacher on one device.  ``cuda``: the native forward (csrc/teacher.hip) in ``precision`` "bf16" or "fp32";
    ``cpu``: ``forward_torch`` (with ``emulate_bf16`` for "bf16").  ``state_dict``: XLMRobertaModel's tensors, with or
    without the ``roberta.`` prefix."""

    def __init__(self, config: TeacherConfig, state_dict: Dict[str, torch.Tensor], device="cuda", precision: str = "bf16"):
        if precision not in PRECISIONS:
            raise ValueError(f"teacher: precision must be one of {sorted(PRECISIONS)}")
        config.validate()
        self.config, self.precision = config, precision
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.params = {k: v.to(self.device).contiguous() for k, v in normalize_state_dict(config, state_dict).items()}
        self._ws: Optional[torch.Tensor] = None
        if self.device.type == "cuda":
            from ._lib import call, fn
            self._desc = config.desc()
            keys = param_keys(config)
            n = int(fn("snx_teacher_param_count")(C.byref(self._desc)))
            if n != len(keys):
                raise RuntimeError(f"teacher: the library counts {n} parameter tensors, the binding {len(keys)}")
            self._ptrs = (C.c_void_p * n)(*[self.params[k].data_ptr() for k in keys])
            nbytes = int(fn("snx_teacher_weight_cache_bytes")(C.byref(self._desc)))
            with torch.cuda.device(self.device):
                self._wcache = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
                call("snx_teacher_weight_cache_refresh", C.byref(self._desc), self._ptrs,
                     C.c_void_p(self._wcache.data_ptr()), self._stream())

    @staticmethod
    def _stream() -> C.c_void_p:
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    @classmethod
    def from_pretrained(cls, model_dir: str, device="cuda", precision: str = "bf16") -> "TeacherEncoder":
        """Read a local HF / sentence-transformers directory: ``config.json`` (model_type xlm-roberta), ``model.safetensors``
        or ``pytorch_model.bin``; a ``1_Pooling/config.json`` must describe CLS pooling."""
        if not isinstance(model_dir, (str, os.PathLike)) or not os.path.isdir(model_dir):
            raise FileNotFoundError(f"teacher: {model_dir!r} is not a local directory (model names are never resolved)")
        model_dir = os.fspath(model_dir)
        with open(os.path.join(model_dir, "config.json")) as f:
            config = TeacherConfig.from_hf(json.load(f))
        _check_pooling(model_dir)
        return cls(config, _read_weights(model_dir), device, precision)

    def to(self, device) -> "TeacherEncoder":
        """An encoder with the same weights on ``device`` (this one when it is there already)."""
        dev = torch.device(device)
        if dev == self.device or (dev.type == self.device.type and dev.index is None):
            return self
        return TeacherEncoder(self.config, self.params, dev, self.precision)

    def _on_my_gpu(self, tokenizer) -> bool:
        """Does ``tokenizer`` return a CSR of ids (``encode_rows``) on this encoder's GPU?"""
        dev = getattr(tokenizer, "device", None)
        if self.device.type != "cuda" or not hasattr(tokenizer, "encode_rows") or not isinstance(dev, torch.device) or \
                dev.type != "cuda":
            return False
        return (dev.index if dev.index is not None else torch.cuda.current_device()) == self.device.index

    @torch.no_grad()
    def encode_tokens(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, normalize: bool = True) -> torch.Tensor:
        """A padded batch [n, S] -> fp32 [n, hidden] on the encoder's device: the CLS row of every sequence (its first
        unmasked token), L2-normalised unless ``normalize`` is False.  Padding is removed before the forward."""
        if self.device.type != "cuda":
            cls, emb = forward_torch(self.config, self.params, input_ids, attention_mask,
                                     emulate_bf16=self.precision == "bf16")
            return emb if normalize else cls
        ids, mask, pos = _check_batch(self.config, input_ids, attention_mask)
        keep = mask.bool()
        lens = mask.sum(dim=1)
        cu = torch.zeros(int(ids.shape[0]) + 1, dtype=torch.int32, device=lens.device)
        cu[1:] = torch.cumsum(lens, 0)
        dev = self.device
        return self._forward_unpadded(ids[keep].to(dev).contiguous(), pos[keep].to(torch.int32).to(dev).contiguous(),
                                      cu.to(dev), int(lens.max()), normalize)

    def _forward_unpadded(self, ids_u: torch.Tensor, pos_u: torch.Tensor, cu: torch.Tensor, max_len: int,
                          normalize: bool) -> torch.Tensor:
        """The native forward over unpadded token rows, all on the encoder's GPU: ``ids_u`` int64 [T] and ``pos_u`` int32
        [T], sequence after sequence; ``cu`` int32 [n + 1] their offsets; ``max_len`` the longest sequence.  The caller
        has checked ids and positions."""
        from ._lib import call, fn
        dev = self.device
        n, T = int(cu.numel()) - 1, int(ids_u.numel())
        H, prec = self.config.hidden_size, PRECISIONS[self.precision]
        with torch.cuda.device(dev):
            need = int(fn("snx_teacher_workspace_bytes")(C.byref(self._desc), T, n, prec))
            if need <= 0:
                raise RuntimeError("teacher: snx_teacher_workspace_bytes refused the shape")
            if self._ws is None or self._ws.numel() < need:
                self._ws = None                                    # release before growing
                self._ws = torch.empty(need, dtype=torch.uint8, device=dev)
            cls = torch.empty((n, H), dtype=torch.float32, device=dev)
            emb = torch.empty((n, H), dtype=torch.float32, device=dev)
            p = lambda t: C.c_void_p(t.data_ptr())                 # noqa: E731
            call("snx_teacher_forward", C.byref(self._desc), self._ptrs, p(self._wcache), p(ids_u), p(pos_u), p(cu),
                 p(self._ws), p(cls), p(emb), T, n, max_len, prec, self._stream())
        return emb if normalize else cls

    def encode_unpadded(self, ptr: torch.Tensor, ids: torch.Tensor, batch_size: Optional[int] = None,
                        batch_tokens: int = DEFAULT_BATCH_TOKENS, normalize: bool = True) -> torch.Tensor:
        """A CSR of token ids on the encoder's GPU (``ptr`` int64 [n + 1], ``ids`` int64, every row <s> ... </s>: a GPU
        tokenizer's ``encode_rows``) -> fp32 [n, hidden], rows in input order.  The same stable length sort and the same
        batches as ``encode`` forms from lists, so the same bits.  One host read (the row lengths, with the flag of the id
        check); ids and positions are gathered from the CSR on the device."""
        if self.device.type != "cuda" or ptr.device != self.device or ids.device != self.device:
            raise ValueError("teacher: encode_unpadded needs ptr and ids on the encoder's GPU")
        n = int(ptr.numel()) - 1
        out = torch.empty((n, self.config.hidden_size), dtype=torch.float32, device=self.device)
        if n == 0:
            return out
        pad = self.config.pad_token_id
        with torch.cuda.device(self.device):
            ptr, ids = ptr.to(torch.long), ids.to(torch.long)
            row_len = ptr[1:] - ptr[:-1]
            bad = ((ids < 0) | (ids >= self.config.vocab_size)).any().to(torch.long)
            *lens, bad = torch.cat((row_len, bad[None])).tolist()      # the one host read
            if any(l <= 0 for l in lens):
                raise ValueError("teacher: the tokenizer returned an empty sequence")
            if bad:
                raise ValueError(f"teacher: input_ids must lie in [0, {self.config.vocab_size})")
            if max(lens) + pad >= self.config.max_position_embeddings:
                raise ValueError(f"teacher: position {max(lens) + pad} >= max_position_embeddings "
                                 f"{self.config.max_position_embeddings}")
            for batch in _length_batches(lens, batch_size, batch_tokens):
                T = sum(lens[j] for j in batch)
                b = torch.tensor(batch, dtype=torch.long, device=self.device)
                blen = row_len[b]
                cu = torch.zeros(len(batch) + 1, dtype=torch.long, device=self.device)
                torch.cumsum(blen, 0, out=cu[1:])
                within = torch.arange(T, dtype=torch.long, device=self.device) - \
                    torch.repeat_interleave(cu[:-1], blen, output_size=T)
                ids_u = ids[torch.repeat_interleave(ptr[b], blen, output_size=T) + within]
                pos_u = (within + (pad + 1)).to(torch.int32)
                out[b] = self._forward_unpadded(ids_u, pos_u, cu.to(torch.int32), max(lens[j] for j in batch), normalize)
        return out

    def encode(self, texts: Sequence[str], tokenizer: Callable, batch_size: Optional[int] = None, max_length: int = 512,
               batch_tokens: int = DEFAULT_BATCH_TOKENS, normalize: bool = True) -> torch.Tensor:
        """Texts -> fp32 [n, hidden] on the encoder's device, rows in input order.  ``tokenizer``: an HF tokenizer (called
        with ``truncation=True, max_length=max_length, padding=False``; its ``input_ids`` carry <s> ... </s>).  The texts are
        sorted by token length and packed into forwards of at most ``batch_tokens`` token rows (and ``batch_size``
        sequences, when given); a longer single text runs alone.  A tokenizer with ``encode_rows`` that lives on the encoder's
        GPU (snx.unigram.UnigramTokenizer) hands its CSR of ids to ``encode_unpadded``: same batches, same bits, and the ids
        never leave the device."""
        texts = list(texts)
        if int(batch_tokens) < 1 or (batch_size is not None and int(batch_size) < 1):
            raise ValueError("teacher: batch_tokens and batch_size must be positive")
        out = torch.empty((len(texts), self.config.hidden_size), dtype=torch.float32, device=self.device)
        if not texts:
            return out
        if self._on_my_gpu(tokenizer):
            ptr, ids = tokenizer.encode_rows(texts, int(max_length))
            return self.encode_unpadded(ptr, ids, batch_size=batch_size, batch_tokens=batch_tokens, normalize=normalize)
        seqs = [list(s) for s in tokenizer(texts, truncation=True, max_length=int(max_length), padding=False)["input_ids"]]
        if any(len(s) == 0 for s in seqs):
            raise ValueError("teacher: the tokenizer returned an empty sequence")
        for batch in _length_batches([len(s) for s in seqs], batch_size, batch_tokens):
            S = max(len(seqs[j]) for j in batch)
            ids = torch.full((len(batch), S), self.config.pad_token_id, dtype=torch.long)
            mask = torch.zeros((len(batch), S), dtype=torch.long)
            for b, j in enumerate(batch):
                ids[b, :len(seqs[j])] = torch.tensor(seqs[j], dtype=torch.long)
                mask[b, :len(seqs[j])] = 1
            out[torch.tensor(batch, device=self.device)] = self.encode_tokens(ids, mask, normalize=normalize)
        return out
