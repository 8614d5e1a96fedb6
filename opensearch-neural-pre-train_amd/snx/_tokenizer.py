"""What the GPU tokenizers (snx/wordpiece.py, snx/unigram.py) share and neither model owns: loading ``tokenizer.json``, the
frame and the added tokens, the vocabulary's open-addressed table as the device reads it, the call surface of the tree's
tokenizers, and both ends of ``encode_rows``: the texts as a CSR of code points going in, and behind a model's piece
kernels the count -> offsets -> fill -> host-row scatter that makes the ids.

A model supplies ``_parse`` (normalizer, pre-tokenizer, model: ``_vocab``, ``_entries``, ``_max_entry``, ``_unk``),
``_segment_pieces`` (its restatement in plain Python), ``_pack`` and ``_device_pieces`` (its rows and its kernels) and
``decode``."""
from __future__ import annotations

import json
import os
import re
import shutil
import time
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

FILES = ("tokenizer.json", "tokenizer_config.json", "special_tokens_map.json")
_M32 = 0xFFFFFFFF
_ROLES = ("pad", "bos", "eos", "unk", "cls", "sep", "mask")


def entry_hash(cont: int, cps: Sequence[int]) -> int:
    """The hash of a vocabulary key as include/snx.h states it (32-bit arithmetic)."""
    h = 0
    for c in cps:
        h = (h * 0x9E3779B1 + c + 1) & _M32
    x = h ^ (0x85EBCA6B if cont else 0) ^ ((len(cps) * 0xC2B2AE35) & _M32)
    x ^= x >> 16
    x = (x * 0x7FEB352D) & _M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & _M32
    x ^= x >> 16
    return x


def _content(tok) -> Optional[str]:
    if isinstance(tok, str):
        return tok
    if isinstance(tok, dict) and isinstance(tok.get("content"), str):
        return tok["content"]
    return None


def _refuse(field: str, why: str):
    raise ValueError(f"tokenizer.json: {field}: {why}")


class RowTokenizer:
    """``Model.from_pretrained(dir, device="cuda")``; the call surface of the tree's tokenizers."""

    _factory_name = ""                 # the prefix create_tokenizer takes for the host form of this model
    _added_refused: Tuple[str, ...] = ()                       # fields of an added token that must not be set

    def __init__(self, spec: dict, device="cuda", table_size: Optional[int] = None, config: Optional[dict] = None,
                 special_tokens_map: Optional[dict] = None, source_dir: Optional[str] = None):
        self.device = torch.device(device)
        self._pid = os.getpid()
        self._source_dir = source_dir
        self._spec = spec
        self._files = {"tokenizer_config.json": config, "special_tokens_map.json": special_tokens_map}
        self._parse(spec)
        self._parse_template(spec)
        self._parse_added(spec)
        self._roles(config or {}, special_tokens_map or {})
        self.model_max_length = int((config or {}).get("model_max_length", 0) or 0) or None
        E = len(self._entries)
        if table_size is None:
            table_size = 1
            while table_size < 2 * max(E, 1):
                table_size <<= 1
        table_size = int(table_size)
        if table_size < max(E, 1) or table_size & (table_size - 1):
            raise ValueError(f"{type(self).__name__}: table_size must be a power of two >= the {E} vocabulary entries")
        self.table_size = table_size
        self._state = None
        self.last_stats = {"rows": 0, "host_rows": 0, "pack_s": 0.0, "device_s": 0.0}

    # ------------------------------------------------------------------------------------------------ loading
    @classmethod
    def from_pretrained(cls, path: str, device="cuda", table_size: Optional[int] = None):
        """Reads ``tokenizer.json`` only (plus the two files that name the special tokens).  A directory without it is
        refused: from a bare ``vocab.txt`` transformers derives a BertTokenizer with a different pipeline."""
        tj = os.path.join(path, "tokenizer.json")
        if not os.path.isfile(tj):
            raise ValueError(f"{path}: tokenizer.json not found: the pipeline is read from tokenizer.json alone (a vocab.txt "
                             "is not enough, transformers derives a different pipeline from it)")
        with open(tj, encoding="utf-8") as f:
            spec = json.load(f)
        extra = []
        for name in FILES[1:]:
            p = os.path.join(path, name)
            extra.append(json.load(open(p, encoding="utf-8")) if os.path.isfile(p) else None)
        return cls(spec, device=device, table_size=table_size, config=extra[0], special_tokens_map=extra[1],
                   source_dir=path)

    def _parse_template(self, spec: dict) -> None:
        """The frame ``<special> $A <special>`` of post_processor -> ``_bos``, ``_eos``."""
        post = spec.get("post_processor")
        if not isinstance(post, dict) or post.get("type") != "TemplateProcessing":
            _refuse("post_processor", f"type {post.get('type') if isinstance(post, dict) else post!r} is not supported, only "
                    "TemplateProcessing")
        single = post.get("single") or []
        names = []
        ok = len(single) == 3
        for i, item in enumerate(single if ok else []):
            key = "Sequence" if i == 1 else "SpecialToken"
            if not isinstance(item, dict) or key not in item or (i == 1 and item[key].get("id") != "A"):
                ok = False
                break
            names.append(item[key].get("id"))
        if not ok:
            _refuse("post_processor.single", "the template must be <special> $A <special>")
        frame = []
        for name in (names[0], names[2]):
            ids = ((post.get("special_tokens") or {}).get(name) or {}).get("ids")
            if not isinstance(ids, list) or len(ids) != 1:
                _refuse("post_processor.special_tokens", f"{name!r} must have exactly one id")
            frame.append(int(ids[0]))
        self._bos, self._eos = frame

    def _parse_added(self, spec: dict) -> None:
        """``added_tokens``; a token with a field of ``_added_refused`` set goes to the model's ``_refuse_added(index,
        field, content)``, which words the refusal."""
        self._added: Dict[str, int] = {}
        for i, a in enumerate(spec.get("added_tokens") or []):
            for field in self._added_refused:
                if a.get(field):
                    self._refuse_added(i, field, a.get("content"))
            if a.get("content"):
                self._added[str(a["content"])] = int(a["id"])
        # leftmost-longest, as the library's matcher: at one position the longer content is tried first
        alts = sorted(self._added, key=len, reverse=True)
        self._added_re = re.compile("|".join(re.escape(a) for a in alts)) if alts else None
        self._first_chars = frozenset(a[0] for a in alts)
        self._id_to_token: Dict[int, str] = {v: k for k, v in self._vocab.items()}
        self._id_to_token.update({v: k for k, v in self._added.items()})

    def _roles(self, config: dict, smap: dict) -> None:
        for role in _ROLES:
            text = _content(config.get(f"{role}_token")) or _content(smap.get(f"{role}_token"))
            tid = None
            if text is not None:
                tid = self._added.get(text, self._vocab.get(text))
            setattr(self, f"{role}_token", text)
            setattr(self, f"{role}_token_id", tid)
        if self.bos_token_id is None:
            self.bos_token_id = self._bos
        if self.eos_token_id is None:
            self.eos_token_id = self._eos
        if self.unk_token_id is None:
            self.unk_token_id = self._unk

    # ------------------------------------------------------------------------------------------------ host restatement
    def host_pieces(self, text: str) -> List[int]:
        """The pieces of one text without the frame: added tokens are cut out of the raw text, the rest is normalized,
        split into words and matched."""
        if self._added_re is None:
            return self._segment_pieces(text)
        out: List[int] = []
        at = 0
        for m in self._added_re.finditer(text):
            if m.start() > at:
                out.extend(self._segment_pieces(text[at:m.start()]))
            out.append(self._added[m.group()])
            at = m.end()
        if at < len(text):
            out.extend(self._segment_pieces(text[at:]))
        return out

    def _frame(self, pieces: List[int], max_length: Optional[int]) -> List[int]:
        if max_length is not None:
            pieces = pieces[:max_length - 2]
        return [self._bos] + pieces + [self._eos]

    def host_row(self, text: str, max_length: Optional[int] = None) -> List[int]:
        return self._frame(self.host_pieces(text), max_length)

    def _needs_host(self, text: str) -> bool:
        """Does the raw text hold an added token's content?"""
        if self._added_re is None or not any(c in text for c in self._first_chars):
            return False
        return self._added_re.search(text) is not None

    # ------------------------------------------------------------------------------------------------ device
    def _guard(self) -> None:
        if os.getpid() != self._pid:
            name = type(self).__name__
            raise RuntimeError(f"{name}: this tokenizer was created in another process and a forked process must not touch "
                               "the GPU: tokenize in the parent (DataLoader num_workers=0) or use device=\"cpu\" "
                               f"(create_tokenizer(\"{self._factory_name}:DIR\"))")

    def device_tables(self) -> Dict[str, np.ndarray]:
        """The vocabulary as the device reads it (include/snx.h): slots, ent_ptr, ent_cps, ent_id as int32; a model adds
        its own column."""
        mask = self.table_size - 1
        slots = np.full(self.table_size, -1, dtype=np.int32)
        ent_ptr = np.zeros(len(self._entries) + 1, dtype=np.int32)
        cps: List[int] = []
        for e, (cont, key, _) in enumerate(self._entries):
            k = [ord(ch) for ch in key]
            cps.extend(k)
            ent_ptr[e + 1] = len(cps)
            s = entry_hash(cont, k) & mask
            while slots[s] >= 0:                              # linear probing; table_size >= entries, so a slot is free
                s = (s + 1) & mask
            slots[s] = e
        return dict(slots=slots, ent_ptr=ent_ptr, ent_cps=np.asarray(cps, dtype=np.int32),
                    ent_id=np.asarray([i for _, _, i in self._entries], dtype=np.int32))

    def _device_arrays(self) -> Dict[str, np.ndarray]:
        """Everything the model's kernels read that is built once."""
        return self.device_tables()

    def _device_state(self):
        if self._state is None:
            from .retrieval._common import cuda_device
            dev = cuda_device(self.device)
            st = {k: (torch.from_numpy(np.ascontiguousarray(v)).to(dev) if v.size else None)
                  for k, v in self._device_arrays().items()}
            st.update(dev=dev)
            self._state = st
        return self._state

    @classmethod
    def _texts(cls, texts) -> List[str]:
        texts = list(texts)
        if any(not isinstance(t, str) for t in texts):
            raise ValueError(f"{cls.__name__}: texts must be strings")
        return texts

    @classmethod
    def _max_length(cls, max_length) -> Optional[int]:
        if max_length is None:
            return None
        if isinstance(max_length, bool) or int(max_length) < 2:
            raise ValueError(f"{cls.__name__}: max_length must be >= 2 (the frame alone takes two ids)")
        return int(max_length)

    def encode_rows(self, texts: Sequence[str], max_length: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """The unpadded form: (ptr int64 [n+1], ids int64) on the tokenizer's device, row r = ids[ptr[r]:ptr[r+1]] =
        bos, at most max_length - 2 pieces, eos."""
        return self._encode_rows(texts, max_length)[:2]

    def _pack(self, texts: List[str], **how) -> Tuple[np.ndarray, np.ndarray, List[int]]:
        """The texts as the model's kernels take them: (ptr, code_points, the indices of the host's rows); a host row is
        an empty row to the kernels."""
        raise NotImplementedError

    def _device_pieces(self, st, ptr: np.ndarray, d_ptr, d_cps, max_length, **how):
        """The model's kernels over the uploaded rows -> (in_ptr int64 [n+1], pieces int32 [in_ptr[n]] with -1 where no
        piece starts, cnt int64 [n] the length of every row of ids), as ``snx_wp_fill`` takes them."""
        raise NotImplementedError

    def _encode_rows(self, texts, max_length, **how) -> Tuple[torch.Tensor, torch.Tensor, int]:
        """``encode_rows`` and the length of the longest row, which comes back in the last host read with the total."""
        texts = self._texts(texts)
        max_length = self._max_length(max_length)
        n = len(texts)
        if self.device.type == "cpu":
            t0 = time.perf_counter()
            rows = [self.host_row(t, max_length, **how) for t in texts]
            ptr = np.zeros(n + 1, dtype=np.int64)
            if n:
                np.cumsum([len(r) for r in rows], out=ptr[1:])
            ids = np.fromiter((i for r in rows for i in r), dtype=np.int64, count=int(ptr[-1]))
            self.last_stats = {"rows": n, "host_rows": n, "pack_s": time.perf_counter() - t0, "device_s": 0.0}
            return torch.from_numpy(ptr), torch.from_numpy(ids), max((len(r) for r in rows), default=0)
        self._guard()
        from ._text import csr_to_device
        name = type(self).__name__
        st = self._device_state()
        dev = st["dev"]
        if n >= 2 ** 31:
            raise ValueError(f"{name}: at most 2^31 - 1 texts a call")
        t0 = time.perf_counter()
        ptr, cps, host_idx = self._pack(texts, **how)
        host_rows = [self.host_row(texts[i], max_length) for i in host_idx]
        t1 = time.perf_counter()
        if n == 0:
            self.last_stats = {"rows": 0, "host_rows": 0, "pack_s": t1 - t0, "device_s": 0.0}
            return torch.zeros(1, dtype=torch.long, device=dev), torch.zeros(0, dtype=torch.long, device=dev), 0
        with torch.cuda.device(dev):
            d_ptr, d_cps, _ = csr_to_device(ptr, cps, dev, name, trusted=True)
            in_ptr, pieces, cnt = self._device_pieces(st, ptr, d_ptr, d_cps, max_length, **how)
            return self._finish_rows(in_ptr, pieces, cnt, host_idx, host_rows, t0, t1)

    def _finish_rows(self, in_ptr, pieces, cnt, host_idx: List[int], host_rows: List[List[int]], t0: float, t1: float
                     ) -> Tuple[torch.Tensor, torch.Tensor, int]:
        """Behind the piece kernels: the host rows' lengths into ``cnt``, the offsets, the one host read that sizes the
        ids, ``snx_wp_fill``, the host rows' ids scattered into their spans, and the stream drained for ``last_stats``."""
        from ._lib import call
        from .ops import _p, _stream
        from .retrieval._common import offsets
        dev, n = cnt.device, cnt.numel()
        if host_idx:
            h_idx = torch.tensor(host_idx, dtype=torch.long, device=dev)
            h_len = torch.tensor([len(r) for r in host_rows], dtype=torch.long, device=dev)
            cnt[h_idx] = h_len
        out_ptr = offsets(cnt)
        total, widest = torch.stack((out_ptr[-1], cnt.max())).tolist()          # the host read: total sizes out_ids
        ids = torch.empty(total, dtype=torch.long, device=dev)
        call("snx_wp_fill", _p(in_ptr), _p(pieces), n, _p(out_ptr), self._bos, self._eos, _p(ids), _stream())
        if host_idx:
            flat = np.fromiter((i for r in host_rows for i in r), dtype=np.int64)
            within = np.concatenate([np.arange(len(r), dtype=np.int64) for r in host_rows])
            base = torch.repeat_interleave(out_ptr[h_idx], h_len, output_size=int(flat.size))
            ids[base + torch.from_numpy(within).to(dev)] = torch.from_numpy(flat).to(dev)
        torch.cuda.current_stream().synchronize()
        self.last_stats = {"rows": n, "host_rows": len(host_idx), "pack_s": t1 - t0, "device_s": time.perf_counter() - t1}
        return out_ptr, ids, widest

    # ------------------------------------------------------------------------------------------------ call surface
    def __call__(self, texts: Union[str, Sequence[str]], padding=True, truncation=True, max_length: Optional[int] = None,
                 return_tensors: Optional[str] = "pt"):
        single = isinstance(texts, str)
        if single:
            texts = [texts]
        if return_tensors not in (None, "pt"):
            raise ValueError(f"{type(self).__name__}: return_tensors must be \"pt\" or None")
        if padding not in (True, False, "longest", "max_length"):
            raise ValueError(f"{type(self).__name__}: padding must be True, False, \"longest\" or \"max_length\"")
        limit = (max_length if max_length is not None else self.model_max_length) if truncation else None
        ptr, ids, widest = self._encode_rows(texts, limit)
        n = ptr.numel() - 1
        if not padding or return_tensors is None:
            if padding:
                raise ValueError(f"{type(self).__name__}: padded rows are returned as tensors (return_tensors=\"pt\")")
            p, flat = ptr.tolist(), ids.tolist()
            rows = [flat[p[r]:p[r + 1]] for r in range(n)]
            masks = [[1] * len(r) for r in rows]
            return {"input_ids": rows[0] if single else rows, "attention_mask": masks[0] if single else masks}
        if padding == "max_length":
            if max_length is None:
                raise ValueError(f"{type(self).__name__}: padding=\"max_length\" needs max_length")
            L = int(max_length)
            if widest > L:
                raise ValueError(f"{type(self).__name__}: a row is longer than max_length (truncation=False)")
        else:
            L = widest
        pad = self.pad_token_id if self.pad_token_id is not None else 0
        input_ids = torch.empty((n, L), dtype=torch.long, device=ptr.device)
        mask = torch.empty((n, L), dtype=torch.long, device=ptr.device)
        if ptr.device.type == "cpu":
            lens = ptr[1:] - ptr[:-1]
            col = torch.arange(L, dtype=torch.long)[None, :]
            inside = col < lens[:, None]
            src = (ptr[:-1, None] + col).clamp_(max=max(ids.numel() - 1, 0))
            input_ids.copy_(torch.where(inside, ids[src] if ids.numel() else torch.zeros_like(src), torch.tensor(pad)))
            mask.copy_(inside.long())
        elif n and L:
            self._guard()
            from ._lib import call
            from .ops import _p, _stream
            with torch.cuda.device(ptr.device):
                call("snx_wp_pad", _p(ptr), _p(ids), n, L, pad, _p(input_ids), _p(mask), _stream())
        return {"input_ids": input_ids, "attention_mask": mask}

    def encode(self, text: str, add_special_tokens: bool = True) -> List[int]:
        if self.device.type == "cpu":
            return self.host_row(text) if add_special_tokens else self.host_pieces(text)
        _, ids = self.encode_rows([text])
        ids = ids.tolist()
        return ids if add_special_tokens else ids[1:-1]

    def convert_ids_to_tokens(self, ids):
        if isinstance(ids, (int, np.integer)):
            return self._id_to_token.get(int(ids))
        return [self._id_to_token.get(int(i)) for i in ids]

    def _tokens(self, ids, skip_special_tokens: bool) -> List[str]:
        """The tokens of ``ids`` for ``decode``: unknown ids dropped, and added tokens too on request."""
        if isinstance(ids, torch.Tensor):
            ids = ids.tolist()
        special = set(self._added.values()) if skip_special_tokens else ()
        toks = (self._id_to_token.get(int(i)) for i in ids if int(i) not in special)
        return [t for t in toks if t is not None]

    @property
    def vocab_size(self) -> int:
        """The model's vocabulary without added tokens, as transformers counts it; ``len()`` counts them in."""
        return len(self._vocab)

    def __len__(self) -> int:
        return len(self._id_to_token)

    def get_vocab(self) -> Dict[str, int]:
        return {**self._vocab, **self._added}

    def save_pretrained(self, path: str) -> None:
        """Copies the files the tokenizer was read from (one built from a dict writes that dict)."""
        os.makedirs(path, exist_ok=True)
        if self._source_dir is not None:
            for name in FILES:
                src = os.path.join(self._source_dir, name)
                if os.path.isfile(src) and os.path.abspath(src) != os.path.abspath(os.path.join(path, name)):
                    shutil.copyfile(src, os.path.join(path, name))
            return
        with open(os.path.join(path, "tokenizer.json"), "w", encoding="utf-8") as f:
            json.dump(self._spec, f, ensure_ascii=False)
        for name, body in self._files.items():
            if body is not None:
                with open(os.path.join(path, name), "w", encoding="utf-8") as f:
                    json.dump(body, f, ensure_ascii=False)
