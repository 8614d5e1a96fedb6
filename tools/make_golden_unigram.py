#!/usr/bin/env python3
"""Write tests/golden/g24_unigram/ by RUNNING sentencepiece, transformers and the `tokenizers` library.

    python tools/make_golden_unigram.py

Needs `sentencepiece`, `tokenizers` and `transformers`.  Nothing is read from outside this repository.  Data only:

  tokenizer.json.gz          the tokenizer.json transformers' XLMRobertaTokenizer writes for a SentencePiece Unigram model of
                             2,000 pieces trained here on a seeded synthetic Korean / Latin corpus with the nmt_nfkc rule (the
                             library's real charsmap), vocabulary laid out as XLM-RoBERTa's: <s> <pad> </s> <unk>, the model's
                             pieces from index 3, <mask>; gzipped, tests/unigram_reference.py fixture_dir() unpacks it
  tokenizer_config.json      as transformers saved them (special_tokens_map.json when it writes one)
  cases.json                 {"cases": [{"name", "text", "normalized": the normalizer's output for the text,
                             "ids": {"none" | "8" | "64": the ids tokenizers' encode returns under that max_length}}]}: the
                             named edge rows, one case a line
  random_cases.json.gz       the same form: seeded random rows (tests/unigram_reference.py random_text)
  variants.json.gz           the library's ids (no truncation) for every row above under the old serialized form of the
                             pipeline and with <mask> lstrip: true; the tie vocabulary with the library's ids for its rows,
                             and for the same rows with the normalizer taken out (the charsmap rewrites U+2581 to a space:
                             only so does a literal one reach the pre-tokenizer)

Asserted here, on the library's own output: what the named cases are there for."""
import gzip
import io
import json
import os
import random
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.unigram_reference import (GOLDEN as OUT, MAX_LENGTHS, META, key_of, mask_lstrip_spec, old_form_spec,  # noqa: E402
                                     random_text, tie_pieces, tie_text, vocabulary_pieces, with_vocab)

SEED = 2424
RANDOM_ROWS = 300
TIE_ROWS = 300
LIMIT = 1 << 20                        # bytes a committed file may have
BOS, PAD, EOS, UNK = 0, 1, 2, 3


def corpus(seed: int):
    """Seeded sentences of Korean and Latin words drawn from two Zipf-like lexicons, with digits and punctuation."""
    rng = random.Random(seed)
    syl = [chr(rng.randint(0xAC00, 0xD7A3)) for _ in range(260)]
    ko = ["".join(rng.choice(syl) for _ in range(rng.randint(1, 4))) for _ in range(2500)]
    cv = [c + v for c in "bcdfghjklmnprstvwz" for v in "aeiou"] + ["th", "ing", "er", "on", "st", "qu"]
    la = ["".join(rng.choice(cv) for _ in range(rng.randint(1, 4))) for _ in range(2500)]
    josa = ["은", "는", "이", "가", "을", "를", "의", "에", "에서", "으로", "하다", "했다", "입니다"]
    for _ in range(30000):
        words = []
        for _ in range(rng.randint(3, 14)):
            r = rng.random()
            if r < 0.5:
                w = ko[min(int(rng.paretovariate(0.9)) - 1, len(ko) - 1)] + (rng.choice(josa) if rng.random() < 0.5 else "")
            elif r < 0.9:
                w = la[min(int(rng.paretovariate(0.9)) - 1, len(la) - 1)]
                w = w.capitalize() if rng.random() < 0.1 else w
            elif r < 0.95:
                w = str(rng.randint(0, 9999))
            else:
                w = rng.choice(["(", ")", "-", "\"", "'", "%", "/", ":"])
            words.append(w)
        yield " ".join(words) + rng.choice([".", ".", "?", "!", ","])


def train():
    """-> (pieces [(text, score)] in the model's order, the precompiled charsmap bytes)."""
    import sentencepiece as spm
    from sentencepiece import sentencepiece_model_pb2 as pb
    model = io.BytesIO()
    spm.SentencePieceTrainer.train(sentence_iterator=corpus(SEED), model_writer=model, vocab_size=2000, model_type="unigram",
                                   normalization_rule_name="nmt_nfkc", character_coverage=0.9995, num_threads=1,
                                   input_sentence_size=0, shuffle_input_sentence=False, minloglevel=2)
    proto = pb.ModelProto()
    proto.ParseFromString(model.getvalue())
    pieces = [(p.piece, float(p.score)) for p in proto.pieces]
    assert [p for p, _ in pieces[:3]] == ["<unk>", "<s>", "</s>"] and len(pieces) == 2000
    return pieces, bytes(proto.normalizer_spec.precompiled_charsmap)


def named_cases(encode, tokens, normalize, pieces):
    """(name, text) of every edge row; ``encode(text)`` -> the library's unframed ids, ``tokens(text)`` its pieces,
    ``normalize(text)`` the normalizer's output."""
    known = {p for p, _ in pieces}
    longest = max(len(p) for p in known)
    word = next(p for p in sorted(known) if len(p) == longest and p.startswith(META) and META not in p[1:])
    assert encode(word[1:]) == encode(word) and len(encode(word[1:])) == 1
    unknown = [ch for ch in ("\U0001F600", "\u4e2d", "\u0416", "\u05d0", "\u0e01", "\u2207") if encode(ch)[-1] == UNK]
    assert len(unknown) >= 3, unknown
    u1, u2, u3 = unknown[:3]
    one = [w for w in ("a b c d e f g h".split()) if len(encode(w)) == 1]
    one = one + [p[1:] for p in sorted(known) if p.startswith(META) and len(p) > 2 and len(encode(p[1:])) == 1][:8 - len(one)]
    assert len(one) == 8
    gone = "".join(chr(c) for c in (0x200B, 0x200E, 0xAD, 0x200C, 0xFEFF, 0x7F, 0x01) if normalize(chr(c)) == "")
    assert len(gone) >= 2, gone
    cases = [
        ("empty", ""),
        ("space_only", "   "),
        ("unicode_space_only", "\u3000\xa0\u2028\x85 \t\n\u1680\u2000\u200a\u2029\u202f\u205f"),
        ("normalizes_to_nothing", gone),
        ("fdfa", "\ufdfa"),
        ("fdfa_in_context", "a\ufdfab \ufdfa\ufdfa"),
        ("nbsp", "a\xa0b \xa0 c"),
        ("zero_width_becomes_space", "a\u200bb c\u200ed"),
        ("controls_removed", "a\x01b\x1cc \x7f"),
        ("fullwidth_run", "\uff21\uff22\uff23\u3000\uff11\uff12\uff13\uff01\uff48\uff45\uff4c\uff4c\uff4f"),
        ("enclosed_digit", "\u2460"),
        ("enclosed_digit_in_context", "a\u2460b \u2461\u2462"),
        ("parenthesized_ju", "\u321c"),
        ("parenthesized_ju_in_context", "\u321c\uac80\uc0c9 x\u321c"),
        ("meta_at_start", META + "ab"),
        ("meta_in_the_middle", "ab" + META + "cd"),
        ("meta_doubled", META + META + "ab cd" + META + META),
        ("meta_alone", META),
        ("meta_after_space", "ab " + META + " " + META + "cd"),
        ("unknown_alone", u1),
        ("unknown_consecutive_inside_a_word", "ab" + u1 + u2 + u3 + "cd"),
        ("unknown_in_adjacent_words", u1 + " " + u2 + " " + u3),
        ("unknown_at_word_ends", u1 + "ab" + u2 + " " + u3 + u3),
        ("longest_piece_word", word[1:]),
        ("longest_piece_word_plus_one", word[1:] + word[1]),
        ("longest_piece_word_in_context", "ab " + word[1:] + word[1:] + " cd"),
        ("added_bos", "<s>"),
        ("added_unk", "<unk>"),
        ("added_pad_eos", "<pad>x</s>"),
        ("added_in_context", "hello <mask> world<mask>! <s><s>"),
        ("added_next_to_space", "a <mask> b  <mask>  c"),
        ("added_text_after_normalization", "<s\u200b> <\uff53>"),
        ("combining_acute", "e\u0301"),
        ("combining_acute_in_context", "cafe\u0301 re\u0301sume\u0301"),
        ("decomposed_jamo", "\u1112\u1161\u11ab"),
        ("decomposed_jamo_in_context", "\u1112\u1161\u11ab\u1100\u1173\u11af \uac80\uc0c9"),
        ("compat_jamo", "\u3131\u314f\u3134 \u314e\u314e"),
        ("flag_and_zwj", "\U0001f1f0\U0001f1f7 \U0001f468\u200d\U0001f469\u200d\U0001f467 x"),
        ("devanagari", "\u0928\u092e\u0938\u094d\u0924\u0947 \u0915\u094d\u0937"),
        ("crlf", "a\r\nb\rc\nd"),
        ("c0_controls", "a\x1cb c\x1dd \x01e\x7f"),
        ("pieces_5", " ".join(one[:5])),
        ("pieces_6", " ".join(one[:6])),
        ("pieces_7", " ".join(one[:7])),
        ("cut_inside_a_word", " ".join(one[:4]) + " " + "안녕하세요반갑습니다"),
        ("mixed", "한국어 검색엔진(Search Engine)은 2024년에 100% 빨라졌다… 정말?! OpenSearch의 neural-sparse, 그리고 漢字와 ﬁ."),
        ("cased", "Hello hello HELLO hELLO"),
        ("ligatures_and_fractions", "\ufb01 \ufb00 \xbd \xbe \u2122 \u338f \u337f \u2167"),
        ("leading_trailing_space", "  \t hello  world \n"),
        ("words_257", " ".join(one[(3 * i) % 8] for i in range(257))),
    ]
    n = {name: encode(text) for name, text in cases}
    for name in ("empty", "space_only", "unicode_space_only", "normalizes_to_nothing"):
        assert n[name] == [], name
    assert n["unknown_alone"] == [n["unknown_alone"][0], UNK][-len(n["unknown_alone"]):] and n["unknown_alone"][-1] == UNK
    inside = tokens("ab" + u1 + u2 + u3 + "cd")
    assert n["unknown_consecutive_inside_a_word"].count(UNK) == 1 and u1 + u2 + u3 in inside, inside   # fused within a word
    assert n["unknown_in_adjacent_words"].count(UNK) == 3                                            # not across words
    assert len(n["longest_piece_word"]) == 1 and len(n["longest_piece_word_plus_one"]) > 1
    assert tokens(META + META + "ab")[0] == META
    assert (len(n["pieces_5"]), len(n["pieces_6"]), len(n["pieces_7"])) == (5, 6, 7)
    assert len(n["cut_inside_a_word"]) > 6
    assert n["added_bos"] == [BOS] and n["added_pad_eos"][0] == PAD and n["added_pad_eos"][-1] == EOS
    return cases


def write_json(path, meta, cases):
    """One case a line, so that a change of one row is a change of one line."""
    text = json.dumps(meta)[:-1] + ', "cases": [\n' + ",\n".join(
        json.dumps(c, ensure_ascii=True, separators=(",", ":")) for c in cases) + "\n]}\n"
    assert json.loads(text)["cases"] == cases
    write_text(path, text)


def write_text(path, text):
    if path.endswith(".gz"):
        with open(path, "wb") as f, gzip.GzipFile(fileobj=f, mode="wb", compresslevel=9, mtime=0, filename="") as g:
            g.write(text.encode("utf-8"))
    else:
        with open(path, "w", encoding="utf-8") as f:
            f.write(text)


def main():
    from tokenizers import Tokenizer
    from transformers import XLMRobertaTokenizer
    spm_pieces, charsmap = train()
    vocab = [("<s>", 0.0), ("<pad>", 0.0), ("</s>", 0.0), ("<unk>", 0.0)] + spm_pieces[3:] + [("<mask>", 0.0)]
    assert len({p for p, _ in vocab}) == len(vocab)
    if os.path.isdir(OUT):
        shutil.rmtree(OUT)
    os.makedirs(OUT)
    with tempfile.TemporaryDirectory() as td:
        XLMRobertaTokenizer(vocab=vocab, _spm_precompiled_charsmap=charsmap).save_pretrained(td)
        with open(os.path.join(td, "tokenizer.json"), "rb") as f:
            raw = f.read()
        for name in ("tokenizer_config.json", "special_tokens_map.json"):
            if os.path.isfile(os.path.join(td, name)):
                shutil.copyfile(os.path.join(td, name), os.path.join(OUT, name))
                os.chmod(os.path.join(OUT, name), 0o644)
    write_text(os.path.join(OUT, "tokenizer.json.gz"), raw.decode("utf-8"))
    spec = json.loads(raw.decode("utf-8"))
    assert spec["model"]["type"] == "Unigram" and spec["normalizer"]["type"] == "Precompiled"
    assert [v[0] for v in spec["model"]["vocab"]] == [p for p, _ in vocab]

    lib = Tokenizer.from_str(json.dumps(spec))
    lib.no_truncation()
    lib.no_padding()
    named = named_cases(lambda t: lib.encode(t, add_special_tokens=False).ids,
                        lambda t: lib.encode(t, add_special_tokens=False).tokens, lib.normalizer.normalize_str, vocab)
    rng = random.Random(SEED)
    pieces = vocabulary_pieces(spec)
    rows = [(f"random_{i:03d}", random_text(rng, pieces, 120)) for i in range(RANDOM_ROWS)]
    out = [{"name": n, "text": t, "normalized": lib.normalizer.normalize_str(t), "ids": {}} for n, t in named + rows]
    for m in MAX_LENGTHS:
        if m is None:
            lib.no_truncation()
        else:
            lib.enable_truncation(max_length=m)
        for rec in out:
            rec["ids"][key_of(m)] = lib.encode(rec["text"]).ids
    meta = {"source": "tokenizers.Tokenizer.encode on the tokenizer.json of this directory", "max_lengths": ["none", "8", "64"]}
    write_json(os.path.join(OUT, "cases.json"), meta, out[:len(named)])
    write_json(os.path.join(OUT, "random_cases.json.gz"), {**meta, "seed": SEED}, out[len(named):])

    variants = {}
    for name, fn in (("old_form", old_form_spec), ("mask_lstrip", mask_lstrip_spec)):
        v = Tokenizer.from_str(json.dumps(fn(spec)))
        v.no_truncation()
        variants[name] = {"cases": [{"text": rec["text"], "ids": v.encode(rec["text"]).ids} for rec in out]}
    same = sum(a["ids"] == rec["ids"]["none"] for a, rec in zip(variants["old_form"]["cases"], out))
    assert same == len(out), f"the old form differs on {len(out) - same} rows"
    tp = tie_pieces()
    tie = Tokenizer.from_str(json.dumps(with_vocab(spec, tp)))
    tie.no_truncation()
    trng = random.Random(SEED + 1)
    texts = [tie_text(trng) for _ in range(TIE_ROWS)]
    variants["tie"] = {"pieces": [[p, s] for p, s in tp], "cases": [{"text": t, "ids": tie.encode(t).ids} for t in texts]}
    assert any(UNK in c["ids"] for c in variants["tie"]["cases"])
    # SentencePiece's charsmap rewrites U+2581 to a space, so a literal one reaches the pre-tokenizer only without the
    # normalizer: the same rows through the same pipeline with the normalizer taken out
    bare = with_vocab(spec, tp)
    bare["normalizer"] = None
    bare = Tokenizer.from_str(json.dumps(bare))
    bare.no_truncation()
    assert lib.normalizer.normalize_str(META) == " "
    variants["tie_normalized"] = {"cases": [{"text": t, "ids": bare.encode(t).ids} for t in texts]}
    assert sum(a["ids"] != b["ids"] for a, b in zip(variants["tie"]["cases"], variants["tie_normalized"]["cases"])) > 50
    write_text(os.path.join(OUT, "variants.json.gz"), json.dumps(variants, ensure_ascii=True, separators=(",", ":")))
    sizes = {n: os.path.getsize(os.path.join(OUT, n)) for n in sorted(os.listdir(OUT))}
    assert all(s < LIMIT for s in sizes.values()), sizes
    print(f"wrote {OUT}: {len(named)} named and {len(rows)} random cases, longest piece "
          f"{max(len(p) for p, _ in vocab)} code points, {sizes}")


if __name__ == "__main__":
    main()
