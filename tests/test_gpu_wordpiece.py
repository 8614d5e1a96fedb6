"""The WordPiece tokenizer on the GPU (csrc/wordpiece.hip, snx/wordpiece.py) against the `tokenizers` library's recorded
output (tests/golden/g23_tokenizer) and against the host restatement.  Every comparison is bit for bit on ptr and ids: a
tokenizer has no tolerance.  Nothing here needs `tokenizers` or `transformers`."""
import json
import os
import random

import pytest
import torch

from tests.wordpiece_reference import (MAX_LENGTHS, collision_vocabulary, fast_path_text, key_of, load_cases,
                                       random_text, synthetic_spec, vocabulary_pieces, fixture_dir)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    from snx.wordpiece import WordPieceTokenizer
    return WordPieceTokenizer.from_pretrained(fixture_dir(), device="cuda")


@pytest.fixture(scope="module")
def cpu():
    from snx.wordpiece import WordPieceTokenizer
    return WordPieceTokenizer.from_pretrained(fixture_dir(), device="cpu")


@pytest.fixture(scope="module")
def cases():
    return load_cases()


@pytest.fixture(scope="module")
def pieces():
    return vocabulary_pieces()


def rows_of(ptr, ids):
    assert ptr.dtype == torch.long and ids.dtype == torch.long and ptr.is_cuda and ids.is_cuda
    p, flat = ptr.tolist(), ids.tolist()
    assert p[0] == 0 and p[-1] == len(flat)
    return [flat[p[r]:p[r + 1]] for r in range(len(p) - 1)]


def assert_rows(got, want, names):
    assert len(got) == len(want)
    for g, w, n in zip(got, want, names):
        assert g == w, n


@pytest.mark.parametrize("max_length", MAX_LENGTHS, ids=key_of)
def test_goldens(gpu, cases, max_length):
    texts = [c["text"] for c in cases]
    got = rows_of(*gpu.encode_rows(texts, max_length))
    assert_rows(got, [c["ids"][key_of(max_length)] for c in cases], [c["name"] for c in cases])
    assert gpu.last_stats["rows"] == len(cases)


@pytest.mark.parametrize("max_length", (None, 64), ids=key_of)
def test_random_corpus_equals_the_host_restatement(gpu, cpu, pieces, max_length):
    rng = random.Random(4242)
    texts = [random_text(rng, pieces, 400) for _ in range(2000)]
    got = rows_of(*gpu.encode_rows(texts, max_length))
    assert_rows(got, [cpu.host_row(t, max_length) for t in texts], [repr(t) for t in texts])


def test_padded_call_form(gpu, cases):
    texts = [c["text"] for c in cases]
    for m in (8, 64):
        out = gpu(texts, padding=True, truncation=True, max_length=m, return_tensors="pt")
        ids, mask = out["input_ids"], out["attention_mask"]
        want = [c["ids"][str(m)] for c in cases]
        L = max(len(w) for w in want)
        assert ids.is_cuda and mask.is_cuda and ids.dtype == mask.dtype == torch.long
        assert tuple(ids.shape) == tuple(mask.shape) == (len(cases), L)
        ids, mask = ids.tolist(), mask.tolist()
        for r, w in enumerate(want):
            assert ids[r] == w + [gpu.pad_token_id] * (L - len(w)), cases[r]["name"]
            assert mask[r] == [1] * len(w) + [0] * (L - len(w)), cases[r]["name"]
    lists = gpu(texts[:40], padding=False, truncation=False)
    assert lists["input_ids"] == [c["ids"]["none"] for c in cases[:40]]
    one = gpu("hello world", max_length=64)
    want = gpu.encode("hello world")
    assert want[0] == gpu.bos_token_id and tuple(one["input_ids"].shape) == (1, len(want))
    assert one["input_ids"][0].tolist() == want and one["attention_mask"][0].tolist() == [1] * len(want)


EDGE = ["empty", "space_only", "unicode_space_only", "zero_width_space_is_a_word_character",
        "c0_separator_is_a_word_character", "word_100", "word_101", "prefix_matches_rest_does_not", "three_dots", "cjk_marks",
        "decomposed_jamo", "combining_acute", "added_bos", "added_unk", "added_pad_eos", "bert_mask_is_plain_text", "pieces_5",
        "pieces_6", "pieces_7", "cut_inside_a_word", "words_65", "words_257"]


def test_edge_rows(gpu, cases):
    by_name = {c["name"]: c for c in cases}
    assert all(n in by_name for n in EDGE)
    unk, bos, eos = gpu.unk_token_id, gpu.bos_token_id, gpu.eos_token_id
    # what the rows are there for, on the recorded library output
    assert by_name["empty"]["ids"]["none"] == by_name["unicode_space_only"]["ids"]["none"] == [bos, eos]
    assert by_name["empty"]["text"] == "" and all(ch in by_name["unicode_space_only"]["text"] for ch in "\u3000\u00a0\u2028\u0085")
    assert by_name["zero_width_space_is_a_word_character"]["text"] == "a\u200bb"
    assert len(by_name["zero_width_space_is_a_word_character"]["ids"]["none"]) == 5
    assert by_name["c0_separator_is_a_word_character"]["text"] == "a\x1cb"
    assert by_name["c0_separator_is_a_word_character"]["ids"]["none"] == [bos, unk, eos]
    assert len(by_name["word_100"]["text"]) == 100 and unk not in by_name["word_100"]["ids"]["none"]
    assert len(by_name["word_101"]["text"]) == 101 and by_name["word_101"]["ids"]["none"] == [bos, unk, eos]
    assert by_name["prefix_matches_rest_does_not"]["ids"]["none"] == [bos, unk, eos]
    assert by_name["three_dots"]["text"] == "..." and len(by_name["three_dots"]["ids"]["none"]) == 5
    assert by_name["cjk_marks"]["text"] == "、—」" and len(by_name["cjk_marks"]["ids"]["none"]) == 5
    assert by_name["decomposed_jamo"]["text"] == "\u1112\u1161\u11ab" and by_name["combining_acute"]["text"] == "e\u0301"
    assert by_name["bert_mask_is_plain_text"]["ids"]["none"][1:-1] == gpu.host_pieces("[") + gpu.host_pieces("MASK") + \
        gpu.host_pieces("]")
    assert [len(by_name[f"pieces_{k}"]["ids"]["8"]) for k in (5, 6, 7)] == [7, 8, 8]
    assert len(by_name["cut_inside_a_word"]["ids"]["none"]) > 8 and len(by_name["cut_inside_a_word"]["ids"]["8"]) == 8
    assert len(by_name["words_65"]["text"].split()) == 65 and len(by_name["words_257"]["text"].split()) == 257
    # every edge row alone (n = 1) ...
    for n in EDGE:
        c = by_name[n]
        for m in MAX_LENGTHS:
            assert rows_of(*gpu.encode_rows([c["text"]], m)) == [c["ids"][key_of(m)]], (n, m)
        host = n.startswith("added_")
        assert gpu.last_stats["host_rows"] == (1 if host else 0), n      # host NFC is no fallback
    # ... and all of them in one call, the host's rows between the device's
    for m in MAX_LENGTHS:
        got = rows_of(*gpu.encode_rows([by_name[n]["text"] for n in EDGE], m))
        assert_rows(got, [by_name[n]["ids"][key_of(m)] for n in EDGE], EDGE)
        assert gpu.last_stats == {**gpu.last_stats, "rows": len(EDGE), "host_rows": 3}
    # n = 0
    ptr, ids = gpu.encode_rows([])
    assert ptr.tolist() == [0] and ids.numel() == 0 and ptr.is_cuda
    out = gpu([], padding=True, max_length=8)
    assert tuple(out["input_ids"].shape) == (0, 0)


def test_long_row_goes_through_the_workspace(gpu, cpu, pieces):
    rng = random.Random(77)
    long_text = ""
    while len(long_text) < 20000:
        long_text += random_text(rng, pieces, 400) + " "
    long_text = long_text[:20000]
    assert len(long_text) == 20000 and not gpu._needs_host(long_text)
    over = "가" * 4097                                    # one code point past the LDS form, one unk
    edge = "ab " * 1365 + "c"                            # exactly 4096 code points: the last row of the LDS form
    assert len(edge) == 4096
    texts = ["hello world", long_text, "", "검색 엔진", over, edge, "x" * 5000 + " tail", "끝"]
    for m in (None, 64):
        got = rows_of(*gpu.encode_rows(texts, m))
        assert_rows(got, [cpu.host_row(t, m) for t in texts], [t[:20] for t in texts])
    assert got[4] == [gpu.bos_token_id, gpu.unk_token_id, gpu.eos_token_id]
    assert gpu.last_stats["host_rows"] == 0


def test_collisions_never_decide_an_id():
    from snx.wordpiece import WordPieceTokenizer
    rng = random.Random(99)
    spec = synthetic_spec(collision_vocabulary(rng, 3000, "abcd"))
    probe = WordPieceTokenizer(spec, device="cpu")
    size = 1
    while size < len(probe._entries):
        size <<= 1
    assert len(probe._entries) > 0.7 * size                # long probe chains
    both = {k for c, k, _ in probe._entries if c == 0} & {k for c, k, _ in probe._entries if c == 1}
    assert len(both) > 20
    gpu = WordPieceTokenizer(spec, device="cuda", table_size=size)
    texts = ["".join(rng.choice("abcd  ") for _ in range(rng.randint(0, 60))) for _ in range(500)]
    got = rows_of(*gpu.encode_rows(texts))
    want = [probe.host_row(t) for t in texts]
    assert_rows(got, want, texts)
    assert any(len(w) > 10 and 2 not in w[1:-1] for w in want)


def test_fast_path_needs_no_host_row(gpu, cpu, pieces):
    rng = random.Random(5)
    texts = [fast_path_text(rng, pieces, rng.randint(1, 40)) for _ in range(1000)]
    assert not any("<" in t for t in texts)
    got = rows_of(*gpu.encode_rows(texts, 64))
    assert gpu.last_stats["host_rows"] == 0 and gpu.last_stats["rows"] == 1000
    assert_rows(got, [cpu.host_row(t, 64) for t in texts], texts)


def test_compute_idf_writes_the_same_bytes(tmp_path, pieces):
    from src.train.cli import compute_idf
    rng = random.Random(11)
    path = tmp_path / "train_shard_000.jsonl"
    with open(path, "w", encoding="utf-8") as f:
        for i in range(50):
            rec = {"query": fast_path_text(rng, pieces, 6), "positive": random_text(rng, pieces, 120)}
            if i % 3 == 0:
                rec["negative"] = random_text(rng, pieces, 80) + " <mask>"
            f.write(json.dumps(rec, ensure_ascii=False) + "\n")
    outs = {}
    for kind in ("gpu", "wordpiece"):
        out = tmp_path / kind / "idf"
        os.makedirs(out.parent)
        line = compute_idf.main(["--input", str(path), "--output", str(out), "--tokenizer", f"{kind}:{fixture_dir()}"])
        assert line["vocab_size"] == 50000 and line["num_docs"] >= 90
        outs[kind] = open(str(out) + ".bin", "rb").read()
    assert len(outs["gpu"]) == 4 * 50000 and outs["gpu"] == outs["wordpiece"]


def test_inference_encoder_returns_the_same_dictionaries(gpu, cpu, pieces):
    from benchmark.encoders import NeuralSparseEncoderV33
    from src.model.splade_modern import SPLADEModernBERT
    torch.manual_seed(0)
    model = SPLADEModernBERT(config=dict(vocab_size=50000, hidden_size=256, intermediate_size=384, num_hidden_layers=1,
                                         num_attention_heads=4, pad_token_id=49999))
    rng = random.Random(3)
    texts = [fast_path_text(rng, pieces, rng.randint(1, 30)) for _ in range(12)] + ["", "\ud55c\uad6d\uc5b4 <mask> \uac80\uc0c9", "e\u0301cole"]
    a = NeuralSparseEncoderV33(checkpoint_path=None, device="cuda:0", model=model, tokenizer=gpu, doc_max_length=32)
    b = NeuralSparseEncoderV33(checkpoint_path=None, device="cuda:0", model=model, tokenizer=cpu, doc_max_length=32)
    da, db = a.encode(texts, batch_size=5, top_k=20), b.encode(texts, batch_size=5, top_k=20)
    assert len(da) == len(texts) and any(da) and da == db
    assert a.encode_for_query(texts[0], top_k=10) == b.encode_for_query(texts[0], top_k=10)
