#!/usr/bin/env python3
"""Write tests/golden/g23_tokenizer/ by RUNNING the `tokenizers` library on the reference's tokenizer files.

    python tools/make_golden_tokenizer.py --reference <checkout of the reference project>

Needs the `tokenizers` package.  Data only:

  tokenizer.json.gz          ref:huggingface/v33/tokenizer.json byte for byte, gzipped (the file itself is larger than a
                             committed file may be); tests/wordpiece_reference.py fixture_dir() unpacks it
  tokenizer_config.json      copies of the reference's files (the names and ids of the special tokens)
  special_tokens_map.json
  cases.json                 {"cases": [{"name", "text", "ids": {"none" | "8" | "64": the ids that
                             tokenizers.Tokenizer.from_file(...).encode(text) returns under that max_length}}]}: the
                             named edge rows of the tests, one case a line
  random_cases.json.gz       the same form, gzipped: seeded random rows (tests/wordpiece_reference.py random_text)

Asserted here, on the library's own output: the shapes the named cases are there for (one unk for the 101 code point word
and for the word whose rest has no entry, three marks three words, the piece counts around the cut at max_length 8)."""
import argparse
import gzip
import json
import os
import random
import shutil
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "g23_tokenizer")
SEED = 2323
RANDOM_ROWS = 300
LIMIT = 1 << 20                        # bytes a committed file may have


def named_cases(encode, unk: int):
    """(name, text) of every edge row; ``encode(text)`` -> the library's unframed pieces (used to pick and check them)."""
    one = "a b c d e f g h".split()
    assert all(len(encode(w)) == 1 for w in one)
    tail = None
    for ch in ("\uE000", "\U000F0000", "\u0378", "\U0001FAFF", "\u2FE0"):           # a rest that has no entry
        if encode("the") != [unk] and encode("the" + ch) == [unk]:
            tail = ch
            break
    assert tail is not None, "no word found whose prefix matches and whose rest does not"
    multi = "안녕하세요"
    assert len(encode(multi)) >= 3
    words = ["검색", "engine", "모델", "query", "문서", "index", "토큰", "weight"]
    cases = [
        ("empty", ""),
        ("space_only", "   "),
        ("unicode_space_only", "\u3000\u00a0\u2028\u0085 \t\n\u1680\u2000\u200a\u2029\u202f\u205f"),
        ("zero_width_space_is_a_word_character", "a\u200bb"),
        ("c0_separator_is_a_word_character", "a\x1cb"),
        ("all_c0_separators", "a\x1cb c\x1dd e\x1ef g\x1fh"),
        ("word_100", "x" * 100),
        ("word_101", "x" * 101),
        ("word_101_between_words", "ab " + "가" * 101 + " cd"),
        ("prefix_matches_rest_does_not", "the" + tail),
        ("prefix_matches_rest_does_not_in_context", "say the" + tail + " again"),
        ("three_dots", "..."),
        ("cjk_marks", "、—」"),
        ("ascii_symbols_are_punctuation", "a$b+c<d=e>f^g`h|i~j"),
        ("decomposed_jamo", "\u1112\u1161\u11ab"),
        ("decomposed_jamo_in_context", "\u1112\u1161\u11ab\u1100\u1173\u11af \uac80\uc0c9"),
        ("combining_acute", "e\u0301"),
        ("combining_acute_in_context", "cafe\u0301 re\u0301sume\u0301"),
        ("added_bos", "<s>"),
        ("added_unk", "<unk>"),
        ("added_pad_eos", "<pad>x<\\s>"),
        ("added_in_context", "hello <mask> world <unused7>! <s><s>"),
        ("added_next_to_decomposed", "<cls>e\u0301<sep>"),
        ("template_eos_is_plain_text", "a </s> b"),
        ("bert_mask_is_plain_text", "[MASK]"),
        ("bert_mask_in_context", "the [MASK] of [CLS] and [SEP]"),
        ("pieces_5", " ".join(one[:5])),
        ("pieces_6", " ".join(one[:6])),
        ("pieces_7", " ".join(one[:7])),
        ("cut_inside_a_word", " ".join(one[:4]) + " " + multi),
        ("words_65", " ".join(words[i % len(words)] for i in range(65))),
        ("words_257", " ".join(words[(3 * i) % len(words)] for i in range(257))),
        ("marks_300", ".,!?" * 75),
        ("mixed", "한국어 검색엔진(Search Engine)은 2024년에 100% 빨라졌다… 정말?! OpenSearch의 neural-sparse, 그리고 漢字와 ﬁ."),
        ("cased", "Hello hello HELLO hELLO"),
        ("cjk_run", "東京都は日本の首都です"),
        ("emoji", "좋아요 \U0001F600\U0001F601 \U0001F44D\U0001F3FD"),
        ("fullwidth", "ＡＢＣ　１２３！"),
        ("nfc_singletons", "\u2126 \u212b \u2000a\u2001b"),
        ("leading_trailing_space", "  \t hello  world \n"),
    ]
    counts = {n: len(encode(t)) for n, t in cases}
    assert (counts["pieces_5"], counts["pieces_6"], counts["pieces_7"]) == (5, 6, 7)
    assert counts["cut_inside_a_word"] >= 7 and len(encode(" ".join(one[:4]))) == 4
    assert encode("x" * 101) == [unk] and len(encode("x" * 100)) > 1
    assert encode("the" + tail) == [unk] and encode("a\x1cb") == [unk]
    assert counts["three_dots"] == 3 and counts["cjk_marks"] == 3 and counts["zero_width_space_is_a_word_character"] == 3
    assert counts["ascii_symbols_are_punctuation"] == 19
    assert counts["unicode_space_only"] == 0 and counts["empty"] == 0
    return cases


def write_cases(path, cases, seed=None):
    """One case a line, so that a change of one row is a change of one line."""
    meta = {"source": "tokenizers.Tokenizer.from_file(ref:huggingface/v33/tokenizer.json).encode",
            "max_lengths": ["none", "8", "64"]}
    if seed is not None:
        meta["seed"] = seed
    text = json.dumps(meta)[:-1] + ', "cases": [\n' + ",\n".join(
        json.dumps(c, ensure_ascii=True, separators=(",", ":")) for c in cases) + "\n]}\n"
    assert json.loads(text)["cases"] == cases
    if path.endswith(".gz"):
        with open(path, "wb") as f, gzip.GzipFile(fileobj=f, mode="wb", compresslevel=9, mtime=0, filename="") as g:
            g.write(text.encode("utf-8"))
    else:
        with open(path, "w", encoding="utf-8") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    args = ap.parse_args()
    from tokenizers import Tokenizer
    sys.path.insert(0, ROOT)
    from tests.wordpiece_reference import MAX_LENGTHS, key_of, random_text, vocabulary_pieces

    src = os.path.join(args.reference, "huggingface", "v33")
    if os.path.isdir(OUT):
        shutil.rmtree(OUT)
    os.makedirs(OUT)
    with open(os.path.join(src, "tokenizer.json"), "rb") as f:
        raw = f.read()
    gz = os.path.join(OUT, "tokenizer.json.gz")
    with open(gz, "wb") as f, gzip.GzipFile(fileobj=f, mode="wb", compresslevel=9, mtime=0, filename="") as g:
        g.write(raw)
    with gzip.open(gz, "rb") as f:
        assert f.read() == raw
    for name in ("tokenizer_config.json", "special_tokens_map.json"):
        shutil.copyfile(os.path.join(src, name), os.path.join(OUT, name))
        os.chmod(os.path.join(OUT, name), 0o644)

    spec = json.loads(raw.decode("utf-8"))
    lib = Tokenizer.from_file(os.path.join(src, "tokenizer.json"))
    lib.no_truncation()
    unk = spec["model"]["vocab"][spec["model"]["unk_token"]]
    named = named_cases(lambda t: lib.encode(t, add_special_tokens=False).ids, unk)
    rng = random.Random(SEED)
    pieces = vocabulary_pieces(spec["model"]["vocab"])
    rows = [(f"random_{i:03d}", random_text(rng, pieces, 120)) for i in range(RANDOM_ROWS)]
    out = [{"name": n, "text": t, "ids": {}} for n, t in named + rows]
    for m in MAX_LENGTHS:
        if m is None:
            lib.no_truncation()
        else:
            lib.enable_truncation(max_length=m)
        for rec in out:
            rec["ids"][key_of(m)] = lib.encode(rec["text"]).ids
    write_cases(os.path.join(OUT, "cases.json"), out[:len(named)])
    write_cases(os.path.join(OUT, "random_cases.json.gz"), out[len(named):], seed=SEED)
    sizes = {n: os.path.getsize(os.path.join(OUT, n)) for n in sorted(os.listdir(OUT))}
    assert all(s < LIMIT for s in sizes.values()), sizes
    print(f"wrote {OUT}: {len(named)} named and {len(rows)} random cases, {sizes}")


if __name__ == "__main__":
    main()
