"""Shared by the WordPiece tokenizer's tests and tools/make_golden_tokenizer.py: the fixture (tests/golden/g23_tokenizer
holds the reference's tokenizer.json byte for byte, gzipped; ``fixture_dir`` unpacks it into a tokenizer directory), the
seeded text generators (the pools the host restatement was checked on against the `tokenizers` library) and a
tokenizer.json built from a synthetic vocabulary.  Plain Python, no GPU."""
import atexit
import functools
import gzip
import json
import os
import random
import shutil
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g23_tokenizer")
MAX_LENGTHS = (None, 8, 64)

# (first, last) code point of every pool, or an explicit list
POOLS = {
    "ascii": (0x21, 0x7E), "hangul": (0xAC00, 0xD7A3), "jamo": (0x1100, 0x11FF), "compat_jamo": (0x3130, 0x318F),
    "general_punct": (0x2000, 0x206F), "latin": (0x00A0, 0x024F), "combining": (0x0300, 0x036F),
    "cjk_symbols": (0x3000, 0x303F), "cjk": (0x4E00, 0x9FFF), "emoji": (0x1F300, 0x1F64F), "fullwidth": (0xFF00, 0xFFEF),
    "c0": [0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x1C, 0x1D, 0x1E, 0x1F],
}
POOL_NAMES = sorted(POOLS)


@functools.lru_cache(maxsize=1)
def fixture_dir() -> str:
    """A tokenizer directory made of the golden files alone: tokenizer.json (from tokenizer.json.gz), tokenizer_config.json
    and special_tokens_map.json, in a temporary directory that goes away with the process."""
    out = tempfile.mkdtemp(prefix="g23_tokenizer_")
    atexit.register(shutil.rmtree, out, ignore_errors=True)
    with gzip.open(os.path.join(GOLDEN, "tokenizer.json.gz"), "rb") as src, open(os.path.join(out, "tokenizer.json"), "wb") as f:
        shutil.copyfileobj(src, f)
    for name in ("tokenizer_config.json", "special_tokens_map.json"):
        shutil.copyfile(os.path.join(GOLDEN, name), os.path.join(out, name))
    return out


def load_cases():
    """The named edge rows (cases.json, one case a line) and then the seeded random rows (random_cases.json.gz)."""
    with open(os.path.join(GOLDEN, "cases.json"), encoding="utf-8") as f:
        cases = json.load(f)["cases"]
    with gzip.open(os.path.join(GOLDEN, "random_cases.json.gz"), "rt", encoding="utf-8") as f:
        return cases + json.load(f)["cases"]


def key_of(max_length) -> str:
    return "none" if max_length is None else str(max_length)


def vocabulary_pieces(vocab=None):
    """The entries of ``vocab`` (token -> id; the fixture's by default) as text pieces (the continuation prefix taken
    off), without the entries that look like added tokens."""
    if vocab is None:
        with open(os.path.join(fixture_dir(), "tokenizer.json"), encoding="utf-8") as f:
            vocab = json.load(f)["model"]["vocab"]
    out = []
    for tok in sorted(vocab, key=vocab.get):
        core = tok[2:] if tok.startswith("##") and len(tok) > 2 else tok
        if "<" not in core:
            out.append(core)
    return out


def _pool_char(rng: random.Random, name: str) -> str:
    p = POOLS[name]
    return chr(rng.choice(p)) if isinstance(p, list) else chr(rng.randint(p[0], p[1]))


def random_text(rng: random.Random, pieces, max_cps: int) -> str:
    """A string of 0 .. max_cps code points: vocabulary pieces, spaces and code points of every pool, mixed."""
    target = rng.randint(0, max_cps)
    out, n = [], 0
    while n < target:
        r = rng.random()
        if r < 0.35:
            s = rng.choice(pieces)
        elif r < 0.55:
            s = " "
        else:
            s = _pool_char(rng, rng.choice(POOL_NAMES))
        out.append(s)
        n += len(s)
    return "".join(out)[:target]


def fast_path_text(rng: random.Random, pieces, words: int) -> str:
    """Composed Hangul, ASCII words, CJK and punctuation, no ``<`` and no combining code point: already NFC and free of
    added-token text."""
    out = []
    for _ in range(words):
        r = rng.random()
        if r < 0.4:
            w = "".join(chr(rng.randint(0xAC00, 0xD7A3)) for _ in range(rng.randint(1, 5)))
        elif r < 0.7:
            w = "".join(rng.choice("abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789")
                        for _ in range(rng.randint(1, 9)))
        elif r < 0.8:
            w = "".join(chr(rng.randint(0x4E00, 0x9FFF)) for _ in range(rng.randint(1, 4)))
        elif r < 0.9:
            w = rng.choice(pieces)
            w = "x" if any(0x300 <= ord(c) <= 0x36F or 0x1100 <= ord(c) <= 0x11FF for c in w) else w
        else:
            w = rng.choice(".,!?;:()[]{}'\"-_/\\、。「」—…%&*#@+=^~|$")
        out.append(w)
    return " ".join(out)


def synthetic_spec(vocab: dict, unk: str = "<unk>", bos: str = "<s>", eos: str = "</s>", max_word: int = 100) -> dict:
    """A tokenizer.json of the supported form around ``vocab`` (token -> id; must hold unk, bos and eos)."""
    return {
        "version": "1.0", "truncation": None, "padding": None, "added_tokens": [],
        "normalizer": {"type": "NFC"}, "pre_tokenizer": {"type": "BertPreTokenizer"},
        "post_processor": {
            "type": "TemplateProcessing",
            "single": [{"SpecialToken": {"id": bos, "type_id": 0}}, {"Sequence": {"id": "A", "type_id": 0}},
                       {"SpecialToken": {"id": eos, "type_id": 0}}],
            "pair": [{"Sequence": {"id": "A", "type_id": 0}}, {"Sequence": {"id": "B", "type_id": 1}}],
            "special_tokens": {bos: {"id": bos, "ids": [vocab[bos]], "tokens": [bos]},
                               eos: {"id": eos, "ids": [vocab[eos]], "tokens": [eos]}}},
        "decoder": {"type": "WordPiece", "prefix": "##", "cleanup": True},
        "model": {"type": "WordPiece", "unk_token": unk, "continuing_subword_prefix": "##",
                  "max_input_chars_per_word": max_word, "vocab": dict(vocab)},
    }


def collision_vocabulary(rng: random.Random, entries: int = 3000, alphabet: str = "abcd"):
    """``entries`` random keys of 1 .. 6 letters over ``alphabet``, about a third of them continuations, some in both
    forms; plus the three frame tokens.  -> token -> id."""
    vocab = {"<s>": 0, "</s>": 1, "<unk>": 2}
    while len(vocab) < entries:
        core = "".join(rng.choice(alphabet) for _ in range(rng.randint(1, 6)))
        r = rng.random()
        for tok in ((core,) if r < 0.6 else ("##" + core,) if r < 0.9 else (core, "##" + core)):
            if tok not in vocab and len(vocab) < entries:
                vocab[tok] = len(vocab)
    return vocab
