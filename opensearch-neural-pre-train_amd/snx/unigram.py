"""The dense teacher's tokenizer on the GPU (csrc/unigram.hip, include/snx.h "Unigram tokenizer"): what
``tokenizers.Tokenizer.from_file(tokenizer.json)`` returns for XLM-RoBERTa's pipeline (normalizer ``Precompiled``, that is
SentencePiece's nmt_nfkc charsmap; ``WhitespaceSplit`` + ``Metaspace``; a SentencePiece Unigram model; template
``<s> $A </s>``), id for id.

The rules, as the library applies them:

1. Added tokens are cut out of the raw text first, leftmost-longest.  ``lstrip`` / ``rstrip`` only move white space into
   the cut, and white space is dropped by the split that follows: they change no id and are accepted.
2. ``Precompiled``: the text is walked by extended grapheme cluster.  A cluster of fewer than 6 UTF-8 bytes is looked up
   whole in the charsmap's trie with a common-prefix search and the FIRST (shortest) hit replaces the whole cluster;
   otherwise every code point of the cluster is looked up on its own and replaced or kept.  A row without a code point
   that can join a cluster (Grapheme_Cluster_Break Extend, ZWJ, SpacingMark, Prepend, L, V, T, CR, LF, Regional_Indicator)
   therefore normalizes code point by code point: that is the device's row.
3. The normalized text is split at Rust's ``char::is_whitespace``; a word receives a leading U+2581 unless it begins
   with one, and is cut before every further U+2581.
   SentencePiece's charsmaps rewrite U+2581 itself to a space, so behind them a literal one never arrives here;
   ``encode_rows(..., normalized=True)`` takes texts past the normalizer and is how the rule is tested.
4. Unigram per word, scores in float64: ``unk_score = min(scores) - 10``; for ``st`` ascending a piece ``w[st:en]`` offers
   ``score + best[st]`` and replaces ``best[en]`` only when that is unset or strictly smaller; without a piece of one code
   point at ``st`` the unknown offers ``unk_score + best[st]`` to ``st + 1`` the same way.  Consecutive unknowns of ONE word
   fuse into one id.
5. ``<s>``, at most ``max_length - 2`` pieces, ``</s>``.

Who does what.  The host parses the charsmap once into a map code point -> replacement and builds the table of joining
code points from the ``regex`` module's ``\\p{GCB=...}`` properties.  A row that holds an added token's text or any joining
code point is a HOST ROW: ``host_pieces``, the full restatement in plain Python with clusters from ``regex``'s ``\\X``,
tokenizes it and its ids are scattered into the CSR.  Every other row is the device's.  ``device="cpu"`` runs the
restatement for every row and needs neither ``transformers`` nor ``tokenizers`` nor ``sentencepiece``.

``regex`` follows the Unicode version it was built with; the library's cluster rules (the unicode-segmentation crate) may
be of another version and then differ at the edges (new Extend or Prepend characters, the Indic conjunct rule).  The
goldens (tests/golden/g24_unigram) pin the rows they list.

The published BGE-M3 file has, from memory, the older serialized form (``Sequence[Precompiled, Replace " {2,}"]``,
Metaspace with ``add_prefix_space``); the loader accepts it, but parity on that file itself is unverified: it is not
available offline."""
from __future__ import annotations

import base64
import functools
import os  # noqa: F401  (the fork guard's os.getpid is reached through this module too)
import re
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _text
from ._tokenizer import RowTokenizer, _refuse
from .wordpiece import WHITE_SPACE

META = "\N{LOWER ONE EIGHTH BLOCK}"    # U+2581
MAX_PIECE = 32                         # longest piece on the device, in code points (UG_MAX_PIECE of csrc/unigram.hip)
UNK_PENALTY = 10.0
_JOINING = ("Extend", "ZWJ", "SpacingMark", "Prepend", "L", "V", "T", "CR", "LF", "Regional_Indicator")
_SPACE_RE = re.compile("[" + "".join(re.escape(chr(c)) for c in WHITE_SPACE) + "]+")
_UNIT_RE = re.compile(META + "[^" + META + "]*")


def _regex():
    try:
        import regex
    except ImportError as e:
        raise ImportError("UnigramTokenizer: the Precompiled normalizer walks the text by extended grapheme cluster and the "
                          "`regex` module supplies the clusters (\\X) and the Grapheme_Cluster_Break properties; install "
                          "`regex` (it is installed wherever `transformers` is)") from e
    return regex


@functools.lru_cache(maxsize=1)
def joining_table() -> np.ndarray:
    """uint8 [0x110000]: 1 for a code point that can join an extended grapheme cluster with a neighbour."""
    regex = _regex()
    pat = regex.compile("[" + "".join(r"\p{GCB=%s}" % g for g in _JOINING) + "]")
    text = "".join(chr(c) for c in range(0x110000) if not 0xD800 <= c < 0xE000)
    t = np.zeros(0x110000, dtype=np.uint8)
    t[[ord(ch) for ch in pat.findall(text)]] = 1
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=1)
def _joining_re():
    """A character class of the joining code points, as ranges."""
    t = joining_table()
    idx = np.flatnonzero(t)
    cuts = np.flatnonzero(np.diff(idx) != 1)
    lo = idx[np.concatenate(([0], cuts + 1))]
    hi = idx[np.concatenate((cuts, [idx.size - 1]))]
    return re.compile("[" + "".join(re.escape(chr(a)) + "-" + re.escape(chr(b)) for a, b in zip(lo, hi)) + "]")


class Charsmap:
    """SentencePiece's precompiled charsmap: a uint32 trie size, a darts-clone double array of that many bytes, and a pool
    of NUL-separated UTF-8 replacements."""

    def __init__(self, blob: bytes):
        if len(blob) < 4:
            _refuse("normalizer.precompiled_charsmap", "shorter than its size field")
        size = int.from_bytes(blob[:4], "little")
        if size % 4 or 4 + size > len(blob):
            _refuse("normalizer.precompiled_charsmap", "the trie size does not fit the blob")
        self.units = np.frombuffer(blob, dtype="<u4", count=size // 4, offset=4)
        self.pool = blob[4 + size:]
        self._units = self.units.tolist()

    def _replacement(self, index: int) -> str:
        end = self.pool.find(b"\0", index)
        return self.pool[index:end if end >= 0 else len(self.pool)].decode("utf-8")

    def transform(self, chunk: bytes) -> Optional[str]:
        """The replacement of the FIRST (shortest) key that is a prefix of ``chunk``, None without one."""
        u = self._units
        if not u:
            return None
        unit = u[0]
        pos = (unit >> 10) << ((unit & 0x200) >> 6)
        for c in chunk:
            if c == 0:
                return None
            pos ^= c
            if pos >= len(u):
                return None
            unit = u[pos]
            if unit & 0x800000FF != c:
                return None
            pos ^= (unit >> 10) << ((unit & 0x200) >> 6)
            if (unit >> 8) & 1:
                return self._replacement(u[pos] & 0x7FFFFFFF) if pos < len(u) else None
        return None

    @functools.cached_property
    def code_point_map(self) -> Tuple[np.ndarray, np.ndarray]:
        """(nmap int32 [0x110000], pool int32): nmap[c] = -1 when c is kept, else offset << 5 | length of its replacement
        in ``pool`` (code points).  All code points walk the trie at once, a UTF-8 byte a step."""
        u = self.units.astype(np.int64)
        cp = np.arange(0x110000, dtype=np.int64)
        nb = np.where(cp < 0x80, 1, np.where(cp < 0x800, 2, np.where(cp < 0x10000, 3, 4)))
        byte = np.zeros((4, cp.size), dtype=np.int64)
        byte[0] = np.select([nb == 1, nb == 2, nb == 3], [cp, 0xC0 | cp >> 6, 0xE0 | cp >> 12], 0xF0 | cp >> 18)
        for k in (1, 2, 3):
            byte[k] = 0x80 | (cp >> (6 * np.maximum(nb - 1 - k, 0))) & 0x3F
        offset = lambda x: (x >> 10) << ((x & 0x200) >> 6)          # noqa: E731
        alive = (cp > 0) & ~((cp >= 0xD800) & (cp < 0xE000))
        pos = np.full(cp.size, offset(int(u[0])) if u.size else 0, dtype=np.int64)
        value = np.full(cp.size, -1, dtype=np.int64)
        for k in range(4):
            step = alive & (k < nb)
            pos = np.where(step, pos ^ byte[k], pos)
            ok = step & (pos < u.size)
            unit = u[np.where(ok, pos, 0)]
            ok &= (unit & 0x800000FF) == byte[k]
            alive &= ok | ~step
            pos = np.where(ok, pos ^ offset(unit), pos)
            leaf = ok & ((unit >> 8) & 1 == 1) & (pos < u.size) & (value < 0)
            value = np.where(leaf, u[np.where(leaf, pos, 0)] & 0x7FFFFFFF, value)
            # a hit on a proper prefix of the UTF-8 form would be a key that is no text: the first hit is the last byte's
            alive &= ~leaf
        nmap = np.full(cp.size, -1, dtype=np.int32)
        pool: List[int] = []
        seen: Dict[int, int] = {}
        for c in np.flatnonzero(value >= 0).tolist():
            v = int(value[c])
            if v not in seen:
                rep = [ord(ch) for ch in self._replacement(v)]
                if len(rep) > 31:
                    _refuse("normalizer.precompiled_charsmap", f"the replacement of U+{c:04X} has more than 31 code points")
                seen[v] = len(pool) << 5 | len(rep)
                pool.extend(rep)
            nmap[c] = seen[v]
        return nmap, np.asarray(pool, dtype=np.int32)

    @functools.cached_property
    def _by_char(self) -> Dict[int, str]:
        nmap, pool = self.code_point_map
        return {c: "".join(map(chr, pool[nmap[c] >> 5:(nmap[c] >> 5) + (nmap[c] & 31)])) for c in np.flatnonzero(nmap >= 0).tolist()}

    def normalize_plain(self, text: str) -> str:
        """Code point by code point: the normalizer's output for a text without joining code points."""
        return text.translate(self._by_char)

    def normalize(self, text: str) -> str:
        """The normalizer's output for any text."""
        if _joining_re().search(text) is None:
            return self.normalize_plain(text)
        out = []
        for cluster in _regex().findall(r"\X", text):
            raw = cluster.encode("utf-8")
            if len(raw) < 6:
                hit = self.transform(raw)
                if hit is not None:
                    out.append(hit)
                    continue
            out.append(cluster.translate(self._by_char))
        return "".join(out)


def _is_double_space_replace(n) -> bool:
    return isinstance(n, dict) and n.get("type") == "Replace" and n.get("pattern") == {"Regex": " {2,}"} and n.get("content") == " "


class UnigramTokenizer(RowTokenizer):
    """``UnigramTokenizer.from_pretrained(dir, device="cuda")``; the call surface of the tree's tokenizers
    (``RowTokenizer``, snx/_tokenizer.py)."""

    _factory_name = "unigram"
    _added_refused = ("normalized", "single_word")

    # ------------------------------------------------------------------------------------------------ loading
    def _parse(self, spec: dict) -> None:
        norm = spec.get("normalizer")
        kind = norm.get("type") if isinstance(norm, dict) else norm
        if kind == "Sequence":
            parts = norm.get("normalizers") or []
            # the Replace of runs of spaces changes no id in front of a white-space split
            if len(parts) == 2 and isinstance(parts[0], dict) and parts[0].get("type") == "Precompiled" and \
                    _is_double_space_replace(parts[1]):
                norm, kind = parts[0], "Precompiled"
        if kind != "Precompiled":
            _refuse("normalizer", f"type {kind!r} is not supported, only Precompiled, alone or in a Sequence with a Replace of "
                    "\" {2,}\" by \" \"")
        try:
            blob = base64.b64decode(norm.get("precompiled_charsmap") or "", validate=True)
        except ValueError:
            _refuse("normalizer.precompiled_charsmap", "is not base64")
        self.charsmap = Charsmap(blob)

        pre = spec.get("pre_tokenizer")
        steps = pre.get("pretokenizers") if isinstance(pre, dict) and pre.get("type") == "Sequence" else None
        if not steps or len(steps) != 2 or any(not isinstance(p, dict) for p in steps) or \
                steps[0].get("type") != "WhitespaceSplit" or steps[1].get("type") != "Metaspace":
            _refuse("pre_tokenizer", "only Sequence[WhitespaceSplit, Metaspace] is supported")
        ms = steps[1]
        if ms.get("replacement", META) != META:
            _refuse("pre_tokenizer.replacement", f"{ms.get('replacement')!r} is not supported, only U+2581")
        if "prepend_scheme" in ms:
            if ms["prepend_scheme"] != "always":
                _refuse("pre_tokenizer.prepend_scheme", f"{ms['prepend_scheme']!r} is not supported, only \"always\"")
        elif not ms.get("add_prefix_space", True):
            _refuse("pre_tokenizer.add_prefix_space", "false is not supported")
        if not ms.get("split", True):
            _refuse("pre_tokenizer.split", "false is not supported")

        model = spec.get("model")
        if not isinstance(model, dict) or model.get("type") != "Unigram":
            _refuse("model.type", f"{model.get('type') if isinstance(model, dict) else model!r} is not supported, only Unigram")
        if model.get("byte_fallback"):
            _refuse("model.byte_fallback", "true is not supported")
        vocab = model.get("vocab")
        if not isinstance(vocab, list) or not vocab or any(not isinstance(v, (list, tuple)) or len(v) != 2 for v in vocab):
            _refuse("model.vocab", "a non-empty list of [piece, score] is required")
        unk = model.get("unk_id")
        if not isinstance(unk, int) or isinstance(unk, bool) or not 0 <= unk < len(vocab):
            _refuse("model.unk_id", f"{unk!r} is not an index of the vocabulary")
        self._vocab: Dict[str, int] = {}
        self._scores: List[float] = []
        for i, (piece, score) in enumerate(vocab):
            if piece in self._vocab:
                _refuse("model.vocab", f"the piece {piece!r} occurs twice (entries {self._vocab[piece]} and {i})")
            self._vocab[str(piece)] = i
            self._scores.append(float(score))
        self._unk = unk
        self._unk_score = min(self._scores) - UNK_PENALTY
        # the device's table leaves out what no word can reach: white space inside, or a U+2581 anywhere but in front
        space = frozenset(chr(c) for c in WHITE_SPACE)
        reach = lambda k: k and META not in k[1:] and not any(ch in space for ch in k)         # noqa: E731
        self._entries = [(0, k, v) for k, v in self._vocab.items() if reach(k)]
        for _, k, _ in self._entries:
            if len(k) > MAX_PIECE:
                _refuse("model.vocab", f"the piece {k!r} has {len(k)} code points, the device's bound is {MAX_PIECE}")
        self._max_entry = max((len(k) for _, k, _ in self._entries), default=1)
        self._longest = max(len(k) for k in self._vocab)
        self._lookup = {k: (v, self._scores[v]) for k, v in self._vocab.items()}

    def _refuse_added(self, index: int, field: str, content) -> None:
        _refuse(f"added_tokens[{index}].{field}", f"{content!r}: true is not supported")

    def _parse_added(self, spec: dict) -> None:
        super()._parse_added(spec)
        _joining_re()                                              # needs `regex`: fail at load time, not at the first row
        self._host_marks = joining_table().copy()
        self._host_marks[[ord(c) for c in self._first_chars]] |= 2

    # ------------------------------------------------------------------------------------------------ host restatement
    def _unit_pieces(self, w: str, out: List[int]) -> None:
        """Viterbi over one word (it begins with U+2581 and holds no other)."""
        n, longest, lookup, unk_score = len(w), self._longest, self._lookup, self._unk_score
        best: List[Optional[float]] = [None] * (n + 1)
        back: List[Tuple[int, int]] = [(0, 0)] * (n + 1)
        best[0] = 0.0
        for st in range(n):
            b = best[st]
            single = False
            for en in range(st + 1, min(n, st + longest) + 1):
                hit = lookup.get(w[st:en])
                if hit is None:
                    continue
                cand = hit[1] + b
                if best[en] is None or cand > best[en]:
                    best[en] = cand
                    back[en] = (st, hit[0])
                if en == st + 1:
                    single = True
            if not single:
                cand = unk_score + b
                if best[st + 1] is None or cand > best[st + 1]:
                    best[st + 1] = cand
                    back[st + 1] = (st, self._unk)
        ids: List[int] = []
        en = n
        while en > 0:
            st, tid = back[en]
            if not (tid == self._unk and ids and ids[-1] == self._unk):     # consecutive unknowns of a word fuse
                ids.append(tid)
            en = st
        out.extend(reversed(ids))

    def _normalized_pieces(self, text: str) -> List[int]:
        out: List[int] = []
        for word in _SPACE_RE.split(text):
            if not word:
                continue
            if not word.startswith(META):
                word = META + word
            for unit in _UNIT_RE.findall(word):
                self._unit_pieces(unit, out)
        return out

    def _segment_pieces(self, text: str) -> List[int]:
        return self._normalized_pieces(self.charsmap.normalize(text))

    def host_row(self, text: str, max_length: Optional[int] = None, normalized: bool = False) -> List[int]:
        return self._frame(self._normalized_pieces(text) if normalized else self.host_pieces(text), max_length)

    def normalize(self, text: str) -> str:
        """The normalizer's output for ``text`` (added tokens are not looked for)."""
        return self.charsmap.normalize(text)

    def _needs_host(self, text: str) -> bool:
        """Does the raw text hold an added token's content, or a code point that joins a grapheme cluster?"""
        return _joining_re().search(text) is not None or super()._needs_host(text)

    # ------------------------------------------------------------------------------------------------ device
    def device_tables(self) -> Dict[str, np.ndarray]:
        """The vocabulary as the device reads it (include/snx.h): slots, ent_ptr, ent_cps, ent_id int32, ent_score float64."""
        return dict(super().device_tables(),
                    ent_score=np.asarray([self._scores[i] for _, _, i in self._entries], dtype=np.float64))

    def _device_arrays(self) -> Dict[str, np.ndarray]:
        nmap, pool = self.charsmap.code_point_map
        return dict(self.device_tables(), nmap=nmap, pool=pool)

    def encode_rows(self, texts: Sequence[str], max_length: Optional[int] = None,
                    normalized: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
        """The unpadded form, as ``RowTokenizer.encode_rows``.  ``normalized``: the texts are the normalizer's output
        already; added tokens are not looked for, the charsmap is not applied (on the device: a map that keeps every code
        point) and no row is the host's.  This is the way to a row that holds a literal U+2581: SentencePiece's charsmaps
        rewrite that one to a space.  The device path reads two pairs of numbers back: the size of the normalized text
        (rows grow and shrink under the charsmap) and the size of the ids."""
        return self._encode_rows(texts, max_length, normalized=normalized)[:2]

    def _pack(self, texts: List[str], normalized: bool = False) -> Tuple[np.ndarray, np.ndarray, List[int]]:
        n = len(texts)
        ptr, cps = _text.code_point_csr(texts, "UnigramTokenizer")
        lens = ptr[1:] - ptr[:-1]
        if n and int(lens.max()) >= 2 ** 26:
            raise ValueError("UnigramTokenizer: a text of 2^26 code points or more")
        host_idx: List[int] = []
        if not normalized and cps.size:
            # the host's rows, found on the CSR as a whole: a joining code point, or (for the few rows that hold the first
            # character of an added token) the added token's text
            marks = self._host_marks[cps]                          # 1: joins a cluster, 2: begins an added token
            host = np.zeros(n, dtype=bool)
            host[np.searchsorted(ptr, np.flatnonzero(marks & 1), side="right") - 1] = True
            if self._added_re is not None:
                at = np.flatnonzero(marks & 2)
                for i in np.unique(np.searchsorted(ptr, at, side="right") - 1).tolist():
                    if not host[i] and self._added_re.search(texts[i]) is not None:
                        host[i] = True
            if host.any():                                         # a host row is an empty row to the kernels
                host_idx = np.flatnonzero(host).tolist()
                cps = cps[np.repeat(~host, lens)]
                ptr = np.zeros(n + 1, dtype=np.int64)
                np.cumsum(np.where(host, 0, lens), out=ptr[1:])
        return ptr, cps, host_idx

    def _device_pieces(self, st, ptr: np.ndarray, d_ptr, d_cps, max_length, normalized: bool = False):
        from ._lib import call
        from .ops import _p, _stream
        from .retrieval._common import offsets, workspace
        dev, n = st["dev"], ptr.size - 1
        nlen = torch.empty(n, dtype=torch.long, device=dev)
        if normalized and "keep" not in st:
            st["keep"] = torch.full((0x110000,), -1, dtype=torch.int32, device=dev)
        nmap = st["keep"] if normalized else st["nmap"]
        call("snx_ug_norm_count", _p(d_ptr), _p(d_cps), n, _p(nmap), _p(nlen), _stream())
        nptr = offsets(nlen)
        ntotal, longest = torch.stack((nptr[-1], nlen.max())).tolist()           # host read 1: sizes the normalized text
        if longest >= 2 ** 31:
            raise ValueError("UnigramTokenizer: a text normalizes to 2^31 code points or more")
        norm = torch.empty(ntotal, dtype=torch.int32, device=dev)
        call("snx_ug_norm_fill", _p(d_ptr), _p(d_cps), n, _p(nmap), _p(st["pool"]), _p(nptr), _p(norm), _stream())
        pieces = torch.empty(ntotal, dtype=torch.int32, device=dev)
        cnt = torch.empty(n, dtype=torch.long, device=dev)
        ws, ws_bytes = workspace("snx_ug_workspace_bytes", dev, longest)
        call("snx_ug_pieces", _p(nptr), _p(norm), n, longest, _p(st["slots"]), self.table_size, _p(st["ent_ptr"]),
             _p(st["ent_cps"]), _p(st["ent_id"]), _p(st["ent_score"]), len(self._entries), self._max_entry, self._unk,
             self._unk_score, -1 if max_length is None else max_length - 2, _p(pieces), _p(cnt), _p(ws), ws_bytes,
             _stream())
        return nptr, pieces, cnt                                                 # host read 2 is _finish_rows'

    # ------------------------------------------------------------------------------------------------ call surface
    def decode(self, ids, skip_special_tokens: bool = False) -> str:
        """The Metaspace decoder: pieces joined, U+2581 read as a space, the leading one dropped."""
        toks = self._tokens(ids, skip_special_tokens)
        if toks and toks[0].startswith(META):
            toks[0] = toks[0][1:]
        return "".join(toks).replace(META, " ")
