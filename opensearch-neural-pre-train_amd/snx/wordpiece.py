"""The model's WordPiece tokenizer on the GPU (csrc/wordpiece.hip, include/snx.h "WordPiece tokenizer"): what
``tokenizers.Tokenizer.from_file(tokenizer.json)`` returns for the pipeline the model ships (ref:huggingface/v33/
tokenizer.json: normalizer NFC, BertPreTokenizer, WordPiece, template ``<s> $A </s>``), id for id.

The host's part is the text: NFC (``unicodedata``), the rows as a CSR of code points (snx/_text.py), the class table over
all code points and the vocabulary's hash table, both built once.  A row that holds the text of an added token (``<s>``,
``<pad>``, ...) is tokenized here by ``host_pieces``, the same algorithm in plain Python: the library cuts added tokens
out before it normalizes.  ``device="cpu"`` runs that restatement for every row; it needs neither ``transformers`` nor
``tokenizers``.  Loading, the added tokens, the call surface and both ends of ``encode_rows`` are ``RowTokenizer``'s
(snx/_tokenizer.py); what is here is the model."""
from __future__ import annotations

import functools
import os  # noqa: F401  (the fork guard's os.getpid is reached through this module too)
import unicodedata
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from . import _text
from ._tokenizer import FILES, RowTokenizer, _content, _refuse, entry_hash  # noqa: F401  (names of this module too)

# Rust's char::is_whitespace (White_Space), not str.isspace: U+001C..U+001F and U+200B are word characters
WHITE_SPACE = (*range(0x09, 0x0E), 0x20, 0x85, 0xA0, 0x1680, *range(0x2000, 0x200B), 0x2028, 0x2029, 0x202F, 0x205F, 0x3000)
ASCII_PUNCT = (*range(33, 48), *range(58, 65), *range(91, 97), *range(123, 127))
PUNCT_CATEGORIES = frozenset(("Pc", "Pd", "Pe", "Pf", "Pi", "Po", "Ps"))
WORD, SPACE, PUNCT = 0, 1, 2
MAX_WORD = 128                         # bound of max_input_chars_per_word on the device (WP_WORD_MAX of csrc/wordpiece.hip)


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


def code_point_rows(texts: Sequence[str], who: str = "code_point_rows") -> Tuple[np.ndarray, np.ndarray]:
    """The texts AS THEY ARE (no lower, no strip: the tokenizer is cased) as a CSR of code points."""
    return _text.code_point_csr(texts, who)


class WordPieceTokenizer(RowTokenizer):
    """``WordPieceTokenizer.from_pretrained(dir, device="cuda")``; the call surface of the tree's tokenizers."""

    _factory_name = "wordpiece"
    _added_refused = ("normalized", "lstrip", "rstrip", "single_word")

    # ------------------------------------------------------------------------------------------------ loading
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

    def _refuse_added(self, index: int, field: str, content) -> None:
        _refuse("added_tokens", f"{content!r}: normalized / lstrip / rstrip / single_word are not supported")

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

    # ------------------------------------------------------------------------------------------------ device
    def device_tables(self) -> Dict[str, np.ndarray]:
        """The vocabulary as the device reads it (include/snx.h): slots, ent_ptr, ent_cps, ent_cont, ent_id as int32."""
        return dict(super().device_tables(), ent_cont=np.asarray([c for c, _, _ in self._entries], dtype=np.int32))

    def _device_arrays(self) -> Dict[str, np.ndarray]:
        return dict(self.device_tables(), cls=class_table().copy())

    def _pack(self, texts: List[str]) -> Tuple[np.ndarray, np.ndarray, List[int]]:
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
        ptr, cps = _text.code_point_csr(norm, "WordPieceTokenizer")
        if texts and int((ptr[1:] - ptr[:-1]).max()) >= 2 ** 31:
            raise ValueError("WordPieceTokenizer: a text of 2^31 code points or more")
        return ptr, cps, host_idx

    def _device_pieces(self, st, ptr: np.ndarray, d_ptr, d_cps, max_length):
        from ._lib import call
        from .ops import _p, _stream
        from .retrieval._common import workspace
        dev, n = st["dev"], ptr.size - 1
        longest = int((ptr[1:] - ptr[:-1]).max())
        pieces = torch.empty(int(ptr[-1]), dtype=torch.int32, device=dev) if d_cps is not None else None
        cnt = torch.empty(n, dtype=torch.long, device=dev)
        ws, ws_bytes = workspace("snx_wp_workspace_bytes", dev, longest)
        call("snx_wp_pieces", _p(d_ptr), _p(d_cps), n, longest, _p(st["cls"]), _p(st["slots"]), self.table_size,
             _p(st["ent_ptr"]), _p(st["ent_cps"]), _p(st["ent_cont"]), _p(st["ent_id"]), len(self._entries),
             self._max_entry, self._max_word, self._unk, -1 if max_length is None else max_length - 2, _p(pieces),
             _p(cnt), _p(ws), ws_bytes, _stream())
        return d_ptr, pieces, cnt

    # ------------------------------------------------------------------------------------------------ call surface
    def decode(self, ids, skip_special_tokens: bool = False) -> str:
        """The WordPiece decoder: tokens joined by a space, a continuation glued to what precedes it."""
        out = ""
        for tok in self._tokens(ids, skip_special_tokens):
            if out and self._prefix and tok.startswith(self._prefix):
                out += tok[len(self._prefix):]
            else:
                out += (" " if out else "") + tok
        for a, b in ((" .", "."), (" ?", "?"), (" !", "!"), (" ,", ","), (" ' ", "'"), (" n't", "n't"), (" 'm", "'m"),
                     (" 's", "'s"), (" 've", "'ve"), (" 're", "'re")):
            out = out.replace(a, b)
        return out
