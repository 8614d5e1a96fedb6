"""Plain-Python restatement of the corpus preparation (include/snx.h "Corpus preparation", src.preprocessing.mlm_data):
the flat rule over code points, written from the rule and not from the reference's regular expressions.  The host tests
hold it to the golden g25 (the reference's own functions); the GPU tests hold the kernels to it.

Rules, per document: (1) a blank (U+0020, U+0009) whose predecessor is a blank is dropped, a kept one becomes U+0020;
(2) a maximal run of two or more U+000A separates and is removed, a single one stays; (3) every piece is stripped of
``str.isspace`` code points at both ends, an empty one is dropped; (4) a piece is valid iff ``len >= min_length`` and
``hangul / len >= min_korean_ratio`` in Python's float division.  Over all paragraphs in input order: (5) SHA-256 of the
UTF-8 bytes, first occurrence kept; (6) ``random.seed(seed)``, shuffle, cut at ``max(1, int(n * (1 - val_ratio)))``;
(7) a line is the paragraph with U+000A replaced by U+0020, then U+000A; (8) the two means."""
import hashlib
import random
from typing import Dict, List, Sequence, Tuple

# Python's str.isspace over all of Unicode, as inclusive ranges
SPACE_RANGES = ((0x0009, 0x000D), (0x001C, 0x0020), (0x0085, 0x0085), (0x00A0, 0x00A0), (0x1680, 0x1680),
                (0x2000, 0x200A), (0x2028, 0x2029), (0x202F, 0x202F), (0x205F, 0x205F), (0x3000, 0x3000))
HANGUL_LO, HANGUL_HI = 0xAC00, 0xD7AF


def is_space(c: int) -> bool:
    return any(lo <= c <= hi for lo, hi in SPACE_RANGES)


def is_blank(c: int) -> bool:
    return c == 0x20 or c == 0x09


def is_hangul(c: int) -> bool:
    return HANGUL_LO <= c <= HANGUL_HI


def segment(doc: str) -> List[str]:
    """Rules 1-3: the stripped, non-empty pieces of one document."""
    cps = [ord(ch) for ch in doc]
    n = len(cps)
    pieces: List[List[int]] = [[]]
    i = 0
    while i < n:
        c = cps[i]
        if c == 0x0A:
            j = i
            while j < n and cps[j] == 0x0A:
                j += 1
            if j - i >= 2:
                pieces.append([])
            else:
                pieces[-1].append(c)
            i = j
            continue
        if is_blank(c):
            if not (i > 0 and is_blank(cps[i - 1])):
                pieces[-1].append(0x20)
        else:
            pieces[-1].append(c)
        i += 1
    out = []
    for p in pieces:
        a, b = 0, len(p)
        while a < b and is_space(p[a]):
            a += 1
        while b > a and is_space(p[b - 1]):
            b -= 1
        if b > a:
            out.append("".join(chr(c) for c in p[a:b]))
    return out


def hangul_count(par: str) -> int:
    return sum(1 for ch in par if is_hangul(ord(ch)))


def is_valid(length: int, hangul: int, min_length: int, min_korean_ratio: float) -> bool:
    """Rule 4 on the two counts."""
    if length < min_length:
        return False
    ratio = hangul / length if length else 0.0
    return not ratio < min_korean_ratio


def valid_paragraphs(doc: str, min_length: int, min_korean_ratio: float) -> List[str]:
    return [p for p in segment(doc) if is_valid(len(p), hangul_count(p), min_length, min_korean_ratio)]


def sha256_words(par: str) -> Tuple[int, ...]:
    """The digest as eight 32-bit words, most significant first."""
    d = hashlib.sha256(par.encode("utf-8")).digest()
    return tuple(int.from_bytes(d[4 * j:4 * j + 4], "big") for j in range(8))


def first_equal(keys: Sequence) -> List[int]:
    """first[i] = the smallest index with keys[i]'s value."""
    seen: Dict = {}
    return [seen.setdefault(k if not hasattr(k, "tolist") else tuple(k.tolist()), i) for i, k in enumerate(keys)]


def dedup(paragraphs: Sequence[str]) -> List[str]:
    first = first_equal([sha256_words(p) for p in paragraphs])
    return [p for i, p in enumerate(paragraphs) if first[i] == i]


def split(paragraphs: Sequence[str], val_ratio: float, seed: int) -> Tuple[List[str], List[str]]:
    random.seed(seed)
    shuffled = list(paragraphs)
    random.shuffle(shuffled)
    cut = max(1, int(len(shuffled) * (1 - val_ratio)))
    return shuffled[:cut], shuffled[cut:]


def file_bytes(paragraphs: Sequence[str]) -> bytes:
    return "".join(p.replace("\n", " ") + "\n" for p in paragraphs).encode("utf-8")


def stats(train: Sequence[str], val: Sequence[str]) -> dict:
    every = list(train) + list(val)
    total = len(every)
    return {"total": total, "train": len(train), "val": len(val),
            "mean_length": sum(len(p) for p in every) / total if total else 0,
            "mean_korean_ratio": sum(hangul_count(p) / len(p) for p in every) / total if total else 0}


def pipeline(sources: Sequence[Sequence[str]], min_length: int, min_korean_ratio: float, val_ratio: float, seed: int):
    """Rules 1-8 over ``sources`` (lists of documents) -> (unique, train, val, train bytes, val bytes, stats)."""
    paragraphs = [p for docs in sources for d in docs for p in valid_paragraphs(d, min_length, min_korean_ratio)]
    unique = dedup(paragraphs)
    train, val = split(unique, val_ratio, seed)
    return unique, train, val, file_bytes(train), file_bytes(val), stats(train, val)
