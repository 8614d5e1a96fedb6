"""The model's WordPiece tokenizer on the GPU (csrc/wordpiece.hip, include/snx.h "WordPiece tokenizer"): what
``tokenizers.Tokenizer.from_file(tokenizer.json)`` returns for the pipeline the model ships (ref:huggingface/v33/
tokenizer.json: normalizer NFC, BertPreTokenizer, WordPiece, template ``<s> $A </s>``), id for id.

The host's part is the text: NFC (``unicodedata``), the rows as a CSR of code points, the class table over all code points
and the vocabulary's hash table, both built once.  A row that holds the text of an added token (``<s>``, ``<pad>``, ...)
is tokenized here by ``host_pieces``, the same algorithm in plain Python: the library cuts added tokens out before it
normalizes.  ``device="cpu"`` runs that restatement for every row; it needs neither ``transformers`` nor ``tokenizers``."""
from __future__ import annotations

import functools
import json
import os
import re
import shutil
import time
import unicodedata
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

FILES = ("tokenizer.json", "tokenizer_config.json", "special_tokens_map.json")
# Rust's char::is_whitespace (White_Space), not str.isspace: U+001C..U+001F and U+200B are word characters
WHITE_SPACE = (*range(0x09, 0x0E), 0x20, 0x85, 0xA0, 0x1680, *range(0x2000, 0x200B), 0x2028, 0x2029, 0x202F, 0x205F, 0x3000)
ASCII_PUNCT = (*range(33, 48), *range(58, 65), *range(91, 97), *range(123, 127))
PUNCT_CATEGORIES = frozenset(("Pc", "Pd", "Pe", "Pf", "Pi", "Po", "Ps"))
WORD, SPACE, PUNCT = 0, 1, 2
MAX_WORD = 128                         # bound of max_input_chars_per_word on the device (WP_WORD_MAX of csrc/wordpiece.hip)
_M32 = 0xFFFFFFFF
_ROLES = ("pad", "bos", "eos", "unk", "cls", "sep", "mask")


@functools.lru_cache(maxsize=1)
def class_table() -> np.ndarray:
    """uint8 [0x110000]: 0 a word character, 1 White_Space, 2 punctuation (BertPreTokenizer's two tests)."""
    t = np.zeros(0x110000, dtype=np.uint8)
    cat = unicodedata.category
    for c in range(0x110000):
        if cat(chr(c)) in PUNCT_CATEGORIES:
            t[c] = PUNCT
    t[list(ASCII_PUNCT)] = PUNCT
    t[list(WHITE_SPACE)] = SPACE
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=1)
def _class_bytes() -> bytes:
    return class_table().tobytes()


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


def code_point_rows(texts: Sequence[str], who: str = "code_point_rows") -> Tuple[np.ndarray, np.ndarray]:
    """The texts AS THEY ARE (no lower, no strip: the tokenizer is cased) as a CSR of code points: (ptr int64 [n+1],
    code_points int32).  A lone surrogate raises."""
    ptr = np.zeros(len(texts) + 1, dtype=np.int64)
    if texts:
        np.cumsum(np.fromiter((len(t) for t in texts), dtype=np.int64, count=len(texts)), out=ptr[1:])
    try:
        raw = "".join(texts).encode("utf-32-le")
    except UnicodeEncodeError as e:
        raise ValueError(f"{who}: a text holds a lone surrogate (U+D800..U+DFFF), which has no UTF-8 form") from e
    return ptr, np.frombuffer(raw, dtype="<u4").astype(np.int32)


def _content(tok) -> Optional[str]:
    if isinstance(tok, str):
        return tok
    if isinstance(tok, dict) and isinstance(tok.get("content"), str):
        return tok["content"]
    return None


def _refuse(field: str, why: str):
    raise ValueError(f"tokenizer.json: {field}: {why}")


class WordPieceTokenizer:
    """``WordPieceTokenizer.from_pretrained(dir, device="cuda")``; the call surface of the tree's tokenizers."""

    def __init__(self, spec: dict, device="cuda", table_size: Optional[int] = None, config: Optional[dict] = None,
                 special_tokens_map: Optional[dict] = None, source_dir: Optional[str] = None):
        self.device = torch.device(device)
        self._pid = os.getpid()
        self._source_dir = source_dir
        self._spec = spec
        self._files = {"tokenizer_config.json": config, "special_tokens_map.json": special_tokens_map}
        self._parse(spec)
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
    def from_pretrained(cls, path: str, device="cuda", table_size: Optional[int] = None) -> "WordPieceTokenizer":
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

    def _parse(self, spec: dict) -> None:
        norm = spec.get("normalizer")
        if norm is not None:
            if not isinstance(norm, dict) or norm.get("type") != "NFC":
                if isinstance(norm, dict) and norm.get("lowercase"):
                    _refuse("normalizer.lowercase", "true is not supported (the tokenizer is cased)")
                _refuse("normalizer", f"type {norm.get('type') if isinstance(norm, dict) else norm!r} is not supported, only "
                        "NFC or none")
        self._nfc = norm is not None
        pre = spec.get("pre_tokenizer")
        if isinstance(pre, dict) and pre.get("type") == "Sequence" and len(pre.get("pretokenizers") or []) == 1:
            pre = pre["pretokenizers"][0]
        if not isinstance(pre, dict) or pre.get("type") != "BertPreTokenizer":
            _refuse("pre_tokenizer", f"type {pre.get('type') if isinstance(pre, dict) else pre!r} is not supported, only "
                    "BertPreTokenizer (bare or in a one-element Sequence)")
        model = spec.get("model")
        if not isinstance(model, dict) or model.get("type") != "WordPiece":
            _refuse("model.type", f"{model.get('type') if isinstance(model, dict) else model!r} is not supported, only "
                    "WordPiece")
        vocab = model.get("vocab")
        if not isinstance(vocab, dict) or not vocab:
            _refuse("model.vocab", "a non-empty token -> id object is required")
        prefix = model.get("continuing_subword_prefix", "##")
        if not isinstance(prefix, str):
            _refuse("model.continuing_subword_prefix", "must be a string")
        unk = model.get("unk_token", "[UNK]")
        if unk not in vocab:
            _refuse("model.unk_token", f"{unk!r} is not in the vocabulary")
        max_word = int(model.get("max_input_chars_per_word", 100))
        if not 1 <= max_word <= MAX_WORD:
            _refuse("model.max_input_chars_per_word", f"must be in [1, {MAX_WORD}]")
        self._vocab: Dict[str, int] = {str(k): int(v) for k, v in vocab.items()}
        self._prefix, self._max_word = prefix, max_word
        self._unk = self._vocab[unk]
        # a piece at offset 0 is looked up as it stands, one at a later offset with the prefix in front
        self._cont = {k[len(prefix):]: v for k, v in self._vocab.items() if k.startswith(prefix) and len(k) > len(prefix)}
        # the device's table leaves out what no word can reach: a word is one punctuation mark or a run of word characters
        cls = _class_bytes()
        reach = lambda k: len(k) == 1 and cls[ord(k)] != SPACE or all(cls[ord(ch)] == WORD for ch in k)   # noqa: E731
        self._entries = [(0, k, v) for k, v in self._vocab.items() if k and reach(k)] + \
                        [(1, k, v) for k, v in self._cont.items() if all(cls[ord(ch)] == WORD for ch in k)]
        longest = max((len(k) for _, k, _ in self._entries), default=1)
        self._max_entry = max(1, min(longest, max_word))      # a longer entry can match no word

        self._parse_template(spec)

        self._added: Dict[str, int] = {}
        for a in spec.get("added_tokens") or []:
            if a.get("normalized") or a.get("lstrip") or a.get("rstrip") or a.get("single_word"):
                _refuse("added_tokens", f"{a.get('content')!r}: normalized / lstrip / rstrip / single_word are not supported")
            if a.get("content"):
                self._added[str(a["content"])] = int(a["id"])
        # leftmost-longest, as the library's matcher: at one position the longer content is tried first
        alts = sorted(self._added, key=len, reverse=True)
        self._added_re = re.compile("|".join(re.escape(a) for a in alts)) if alts else None
        self._first_chars = frozenset(a[0] for a in alts)
        self._id_to_token: Dict[int, str] = {v: k for k, v in self._vocab.items()}
        self._id_to_token.update({v: k for k, v in self._added.items()})

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
    def _words(self, text: str) -> List[str]:
        cls = _class_bytes()
        words, cur = [], []
        for ch in text:
            c = cls[ord(ch)]
            if c == WORD:
                cur.append(ch)
                continue
            if cur:
                words.append("".join(cur))
                cur = []
            if c == PUNCT:
                words.append(ch)
        if cur:
            words.append("".join(cur))
        return words

    def _word_pieces(self, word: str) -> List[int]:
        n = len(word)
        if n > self._max_word:
            return [self._unk]
        out, st = [], 0
        while st < n:
            table = self._cont if st else self._vocab
            for en in range(min(n, st + self._max_entry), st, -1):
                tid = table.get(word[st:en])
                if tid is not None:
                    out.append(tid)
                    st = en
                    break
            else:
                return [self._unk]
        return out

    def _segment_pieces(self, text: str) -> List[int]:
        if self._nfc and not unicodedata.is_normalized("NFC", text):
            text = unicodedata.normalize("NFC", text)
        out: List[int] = []
        for w in self._words(text):
            out.extend(self._word_pieces(w))
        return out

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

    def host_row(self, text: str, max_length: Optional[int] = None) -> List[int]:
        pieces = self.host_pieces(text)
        if max_length is not None:
            pieces = pieces[:max_length - 2]
        return [self._bos] + pieces + [self._eos]

    def _needs_host(self, text: str) -> bool:
        """Does the raw text hold an added token's content?"""
        if self._added_re is None or not any(c in text for c in self._first_chars):
            return False
        return self._added_re.search(text) is not None

    # ------------------------------------------------------------------------------------------------ device
    def _guard(self) -> None:
        if os.getpid() != self._pid:
            raise RuntimeError("WordPieceTokenizer: this tokenizer was created in another process and a forked process must "
                               "not touch the GPU: tokenize in the parent (DataLoader num_workers=0) or use device=\"cpu\" "
                               "(create_tokenizer(\"wordpiece:DIR\"))")

    def device_tables(self) -> Dict[str, np.ndarray]:
        """The vocabulary as the device reads it (include/snx.h): slots, ent_ptr, ent_cps, ent_cont, ent_id as int32."""
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
                    ent_cont=np.asarray([c for c, _, _ in self._entries], dtype=np.int32),
                    ent_id=np.asarray([i for _, _, i in self._entries], dtype=np.int32))

    def _device_state(self):
        if self._state is None:
            from .retrieval._common import cuda_device
            dev = cuda_device(self.device)
            st = {k: (torch.from_numpy(v).to(dev) if v.size else None) for k, v in self.device_tables().items()}
            st.update(dev=dev, cls=torch.from_numpy(class_table().copy()).to(dev))
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

    def _encode_rows(self, texts, max_length) -> Tuple[torch.Tensor, torch.Tensor, int]:
        """``encode_rows`` and the length of the longest row, which comes back in the one host read with the total."""
        texts = self._texts(texts)
        max_length = self._max_length(max_length)
        n = len(texts)
        if self.device.type == "cpu":
            t0 = time.perf_counter()
            rows = [self.host_row(t, max_length) for t in texts]
            ptr = np.zeros(n + 1, dtype=np.int64)
            if n:
                np.cumsum([len(r) for r in rows], out=ptr[1:])
            ids = np.fromiter((i for r in rows for i in r), dtype=np.int64, count=int(ptr[-1]))
            self.last_stats = {"rows": n, "host_rows": n, "pack_s": time.perf_counter() - t0, "device_s": 0.0}
            return torch.from_numpy(ptr), torch.from_numpy(ids), max((len(r) for r in rows), default=0)
        self._guard()
        from ._lib import call
        from .ops import _p, _stream
        from .retrieval._common import offsets, workspace
        st = self._device_state()
        dev = st["dev"]
        if n >= 2 ** 31:
            raise ValueError("WordPieceTokenizer: at most 2^31 - 1 texts a call")
        t0 = time.perf_counter()
        host_idx: List[int] = []
        norm: List[str] = []
        for i, t in enumerate(texts):
            if self._needs_host(t):
                host_idx.append(i)
                norm.append("")
            elif self._nfc and not unicodedata.is_normalized("NFC", t):
                norm.append(unicodedata.normalize("NFC", t))
            else:
                norm.append(t)
        host_rows = [self.host_row(texts[i], max_length) for i in host_idx]
        ptr, cps = code_point_rows(norm, "WordPieceTokenizer")
        longest = int((ptr[1:] - ptr[:-1]).max()) if n else 0
        if longest >= 2 ** 31:
            raise ValueError("WordPieceTokenizer: a text of 2^31 code points or more")
        t1 = time.perf_counter()
        if n == 0:
            self.last_stats = {"rows": 0, "host_rows": 0, "pack_s": t1 - t0, "device_s": 0.0}
            return torch.zeros(1, dtype=torch.long, device=dev), torch.zeros(0, dtype=torch.long, device=dev), 0
        with torch.cuda.device(dev):
            d_ptr = torch.from_numpy(ptr).to(dev)
            d_cps = torch.from_numpy(cps).to(dev) if cps.size else None
            pieces = torch.empty(int(cps.size), dtype=torch.int32, device=dev) if cps.size else None
            cnt = torch.empty(n, dtype=torch.long, device=dev)
            ws, ws_bytes = workspace("snx_wp_workspace_bytes", dev, longest)
            call("snx_wp_pieces", _p(d_ptr), _p(d_cps), n, longest, _p(st["cls"]), _p(st["slots"]), self.table_size,
                 _p(st["ent_ptr"]), _p(st["ent_cps"]), _p(st["ent_cont"]), _p(st["ent_id"]), len(self._entries),
                 self._max_entry, self._max_word, self._unk, -1 if max_length is None else max_length - 2, _p(pieces),
                 _p(cnt), _p(ws), ws_bytes, _stream())
            if host_idx:
                h_idx = torch.tensor(host_idx, dtype=torch.long, device=dev)
                h_len = torch.tensor([len(r) for r in host_rows], dtype=torch.long, device=dev)
                cnt[h_idx] = h_len
            out_ptr = offsets(cnt)
            total, widest = torch.stack((out_ptr[-1], cnt.max())).tolist()      # the one host read: total sizes out_ids
            ids = torch.empty(total, dtype=torch.long, device=dev)
            call("snx_wp_fill", _p(d_ptr), _p(pieces), n, _p(out_ptr), self._bos, self._eos, _p(ids), _stream())
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

    def decode(self, ids, skip_special_tokens: bool = False) -> str:
        """The WordPiece decoder: tokens joined by a space, a continuation glued to what precedes it."""
        if isinstance(ids, torch.Tensor):
            ids = ids.tolist()
        special = set(self._added.values())
        out = ""
        for i in ids:
            if skip_special_tokens and int(i) in special:
                continue
            tok = self._id_to_token.get(int(i))
            if tok is None:
                continue
            if out and self._prefix and tok.startswith(self._prefix):
                out += tok[len(self._prefix):]
            else:
                out += (" " if out else "") + tok
        for a, b in ((" .", "."), (" ?", "?"), (" !", "!"), (" ,", ","), (" ' ", "'"), (" n't", "n't"), (" 'm", "'m"),
                     (" 's", "'s"), (" 've", "'ve"), (" 're", "'re")):
            out = out.replace(a, b)
        return out

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
