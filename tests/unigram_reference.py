"""Shared by the Unigram tokenizer's tests and tools/make_golden_unigram.py: the fixture (tests/golden/g24_unigram: a
SentencePiece Unigram model of 2,000 pieces behind the library's nmt_nfkc charsmap, written by transformers'
XLMRobertaTokenizer, gzipped; ``fixture_dir`` unpacks it into a tokenizer directory), the seeded text generators, and the
variants of the pipeline as functions of the fixture's tokenizer.json.  Plain Python, no GPU."""
import atexit
import copy
import functools
import gzip
import json
import os
import random
import shutil
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g24_unigram")
MAX_LENGTHS = (None, 8, 64)
META = "▁"

# (first, last) code point of every pool, or an explicit list
POOLS = {
    "ascii": (0x21, 0x7E), "hangul": (0xAC00, 0xD7A3), "jamo": (0x1100, 0x11FF), "compat_jamo": (0x3130, 0x318F),
    "general_punct": (0x2000, 0x206F), "latin": (0x00A0, 0x024F), "combining": (0x0300, 0x036F),
    "cjk": (0x4E00, 0x9FFF), "emoji": (0x1F300, 0x1F64F), "zwj": [0x200D], "regional": (0x1F1E6, 0x1F1FF),
    "devanagari": (0x0900, 0x097F), "c0": [0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x1C, 0x1D, 0x1E, 0x1F],
    "fullwidth": (0xFF00, 0xFFEF), "fullwidth_ascii": (0xFF01, 0xFF5E), "enclosed": (0x2460, 0x24FF),
    "enclosed_cjk": (0x3200, 0x32FF), "meta": [0x2581],
}
POOL_NAMES = sorted(POOLS)
# pools without a code point that joins a grapheme cluster: rows drawn from these alone are the device's
PLAIN_POOLS = ("ascii", "hangul", "compat_jamo", "latin", "cjk", "fullwidth_ascii", "enclosed", "enclosed_cjk", "meta")


@functools.lru_cache(maxsize=1)
def fixture_dir() -> str:
    """A tokenizer directory made of the golden files alone, in a temporary directory that goes away with the process."""
    out = tempfile.mkdtemp(prefix="g24_unigram_")
    atexit.register(shutil.rmtree, out, ignore_errors=True)
    with gzip.open(os.path.join(GOLDEN, "tokenizer.json.gz"), "rb") as src, open(os.path.join(out, "tokenizer.json"), "wb") as f:
        shutil.copyfileobj(src, f)
    for name in ("tokenizer_config.json", "special_tokens_map.json"):
        if os.path.isfile(os.path.join(GOLDEN, name)):
            shutil.copyfile(os.path.join(GOLDEN, name), os.path.join(out, name))
    return out


@functools.lru_cache(maxsize=1)
def _spec_text() -> str:
    with open(os.path.join(fixture_dir(), "tokenizer.json"), encoding="utf-8") as f:
        return f.read()


def fixture_spec() -> dict:
    """The fixture's tokenizer.json, a fresh object per call."""
    return json.loads(_spec_text())


def load_cases():
    """The named edge rows (cases.json, one case a line) and then the seeded random rows (random_cases.json.gz)."""
    with open(os.path.join(GOLDEN, "cases.json"), encoding="utf-8") as f:
        cases = json.load(f)["cases"]
    with gzip.open(os.path.join(GOLDEN, "random_cases.json.gz"), "rt", encoding="utf-8") as f:
        return cases + json.load(f)["cases"]


def load_variants() -> dict:
    """{"old_form" | "mask_lstrip": {"cases": [{"text", "ids"}]}, "tie": {"pieces": [[piece, score]], "cases": [...]}}."""
    with gzip.open(os.path.join(GOLDEN, "variants.json.gz"), "rt", encoding="utf-8") as f:
        return json.load(f)


def key_of(max_length) -> str:
    return "none" if max_length is None else str(max_length)


def vocabulary_pieces(spec=None):
    """The model's pieces as text (the leading U+2581 taken off), without the special tokens and the bare U+2581."""
    vocab = (spec or fixture_spec())["model"]["vocab"]
    out = []
    for tok, _ in vocab:
        core = tok[1:] if tok.startswith(META) else tok
        if core and "<" not in core:
            out.append(core)
    return out


def _pool_char(rng: random.Random, name: str) -> str:
    p = POOLS[name]
    return chr(rng.choice(p)) if isinstance(p, list) else chr(rng.randint(p[0], p[1]))


def random_text(rng: random.Random, pieces, max_cps: int, pools=POOL_NAMES) -> str:
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
            s = _pool_char(rng, rng.choice(pools))
        out.append(s)
        n += len(s)
    return "".join(out)[:target]


def plain_text(rng: random.Random, pieces, max_cps: int) -> str:
    """``random_text`` over the pools without joining code points, and without ``<``: a row the device tokenizes."""
    return random_text(rng, pieces, max_cps, PLAIN_POOLS).replace("<", "(")


# ---------------------------------------------------------------------------------------------- variants of the pipeline
def old_form_spec(spec: dict) -> dict:
    """The pipeline as older releases of the library serialized it: the Precompiled normalizer followed by a Replace of
    runs of spaces, and the Metaspace pre-tokenizer written with add_prefix_space."""
    s = copy.deepcopy(spec)
    s["normalizer"] = {"type": "Sequence", "normalizers": [
        s["normalizer"], {"type": "Replace", "pattern": {"Regex": " {2,}"}, "content": " "}]}
    pre = s["pre_tokenizer"]["pretokenizers"]
    assert pre[1]["type"] == "Metaspace"
    pre[1] = {"type": "Metaspace", "replacement": META, "add_prefix_space": True}
    return s


def mask_lstrip_spec(spec: dict) -> dict:
    s = copy.deepcopy(spec)
    hit = [a for a in s["added_tokens"] if a["content"] == "<mask>"]
    assert len(hit) == 1
    hit[0]["lstrip"] = True
    return s


def with_vocab(spec: dict, pieces) -> dict:
    """The fixture's pipeline around another vocabulary: <s> <pad> </s> <unk>, ``pieces`` [(text, score)], <mask>."""
    s = copy.deepcopy(spec)
    vocab = [["<s>", 0.0], ["<pad>", 0.0], ["</s>", 0.0], ["<unk>", 0.0]] + [[p, float(x)] for p, x in pieces] + \
            [["<mask>", 0.0]]
    s["model"]["vocab"] = vocab
    s["model"]["unk_id"] = 3
    ids = {tok: i for i, (tok, _) in enumerate(vocab)}
    for a in s["added_tokens"]:
        a["id"] = ids[a["content"]]
    return s


def tie_pieces(seed: int = 46):
    """46 pieces over a, b, c with and without a leading U+2581, scores multiples of -0.5 (sums are exact, so paths tie
    exactly); ``c`` alone is missing, so unk occurs."""
    rng = random.Random(seed)
    cores = [x + y + z for x in ("", *"abc") for y in ("", *"abc") for z in "abc"]
    cand = sorted({c for c in cores if c != "c"} | {META + c for c in cores if c != "c"} | {META})
    picked = sorted(rng.sample(cand, 46))
    for must in ("a", "b", META, META + "a"):
        if must not in picked:
            picked[picked.index(next(p for p in picked if len(p) == 3))] = must
    assert len(set(picked)) == 46 and "c" not in picked
    return [(p, -0.5 * rng.randint(1, 6)) for p in picked]


def tie_text(rng: random.Random, max_cps: int = 24) -> str:
    return "".join(rng.choice("aaabbbc " + META) for _ in range(rng.randint(0, max_cps)))
