"""The Unigram tokenizer on the GPU (csrc/unigram.hip, snx/unigram.py) against the `tokenizers` library's recorded output
(tests/golden/g24_unigram) and against the host restatement, and its CSR of ids through the dense teacher.  Every
comparison is bit for bit on ptr and ids: a tokenizer has no tolerance.  Nothing here needs `tokenizers` or `transformers`."""
import json
import os
import random

import pytest
import torch

from tests.unigram_reference import (MAX_LENGTHS, META, fixture_dir, fixture_spec, key_of, load_cases, load_variants,
                                     plain_text, random_text, tie_text, vocabulary_pieces, with_vocab)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    from snx.unigram import UnigramTokenizer
    return UnigramTokenizer.from_pretrained(fixture_dir(), device="cuda")


@pytest.fixture(scope="module")
def cpu():
    from snx.unigram import UnigramTokenizer
    return UnigramTokenizer.from_pretrained(fixture_dir(), device="cpu")


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
    assert gpu.last_stats["rows"] == len(cases) and 0 < gpu.last_stats["host_rows"] < len(cases)


@pytest.mark.parametrize("max_length", (None, 64), ids=key_of)
def test_random_corpus_equals_the_host_restatement(gpu, cpu, pieces, max_length):
    rng = random.Random(4343)
    texts = [(plain_text if i % 2 else random_text)(rng, pieces, 400) for i in range(2000)]
    got = rows_of(*gpu.encode_rows(texts, max_length))
    assert 500 < gpu.last_stats["host_rows"] < 1500
    assert_rows(got, [cpu.host_row(t, max_length) for t in texts], [repr(t) for t in texts])


DEVICE_EDGE = ["empty", "space_only", "normalizes_to_nothing", "fdfa", "fdfa_in_context", "nbsp",
               "zero_width_becomes_space", "controls_removed", "fullwidth_run", "enclosed_digit", "enclosed_digit_in_context", "parenthesized_ju",
               "parenthesized_ju_in_context", "meta_at_start", "meta_in_the_middle", "meta_doubled", "meta_alone",
               "meta_after_space", "unknown_alone", "unknown_consecutive_inside_a_word", "unknown_in_adjacent_words",
               "unknown_at_word_ends", "longest_piece_word", "longest_piece_word_plus_one", "longest_piece_word_in_context",
               "pieces_5", "pieces_6", "pieces_7", "cut_inside_a_word", "ligatures_and_fractions", "words_257",
               "added_text_after_normalization"]
HOST_EDGE = ["unicode_space_only", "added_bos", "added_in_context", "combining_acute", "decomposed_jamo", "flag_and_zwj",
             "devanagari", "crlf"]


def test_edge_rows(gpu, cases):
    by_name = {c["name"]: c for c in cases}
    edge = DEVICE_EDGE + HOST_EDGE
    assert all(n in by_name for n in edge)
    unk, bos, eos = gpu.unk_token_id, gpu.bos_token_id, gpu.eos_token_id
    ids = lambda n: by_name[n]["ids"]["none"]                 # noqa: E731
    # what the rows are there for, on the recorded library output
    for n in ("empty", "space_only", "unicode_space_only", "normalizes_to_nothing"):
        assert ids(n) == [bos, eos], n
    assert by_name["normalizes_to_nothing"]["text"] != "" and by_name["normalizes_to_nothing"]["normalized"] == ""
    assert by_name["fdfa"]["text"] == chr(0xFDFA) and len(by_name["fdfa"]["normalized"]) == 18
    assert " " in by_name["fdfa"]["normalized"]
    # this charsmap turns the zero-width characters into spaces and removes the C0 controls
    assert by_name["zero_width_becomes_space"]["normalized"] == "a b c d" and by_name["nbsp"]["normalized"] == "a b   c"
    assert by_name["controls_removed"]["normalized"] == "abc "
    assert by_name["fullwidth_run"]["normalized"] == "ABC 123!hello"
    assert by_name["enclosed_digit"]["normalized"] == "1" and by_name["parenthesized_ju"]["normalized"] == "(" + chr(0xC8FC) + ")"
    assert ids("meta_at_start") == gpu.host_row("ab") and ids("meta_in_the_middle") == gpu.host_row("ab cd")
    assert ids("meta_doubled") == gpu.host_row("ab cd") and ids("meta_alone") == [bos, eos]    # the charsmap's U+2581 -> space
    assert ids("unknown_alone")[-2] == unk
    assert ids("unknown_consecutive_inside_a_word").count(unk) == 1 and ids("unknown_in_adjacent_words").count(unk) == 3
    word = by_name["longest_piece_word"]["text"]
    assert len(word) + 1 == gpu._max_entry and len(ids("longest_piece_word")) == 3
    assert len(by_name["longest_piece_word_plus_one"]["text"]) == gpu._max_entry and len(ids("longest_piece_word_plus_one")) > 3
    assert [len(by_name[f"pieces_{k}"]["ids"]["8"]) for k in (5, 6, 7)] == [7, 8, 8]
    assert len(ids("cut_inside_a_word")) > 8 and len(by_name["cut_inside_a_word"]["ids"]["8"]) == 8
    # every edge row alone (n = 1) ...
    for n in edge:
        c = by_name[n]
        for m in MAX_LENGTHS + (2,):
            want = c["ids"][key_of(m)] if m != 2 else [bos, eos]
            assert rows_of(*gpu.encode_rows([c["text"]], m)) == [want], (n, m)
        assert gpu.last_stats["host_rows"] == (1 if n in HOST_EDGE else 0), n
    # ... and all of them in one call, the host's rows between the device's
    order = sorted(edge)
    for m in MAX_LENGTHS:
        got = rows_of(*gpu.encode_rows([by_name[n]["text"] for n in order], m))
        assert_rows(got, [by_name[n]["ids"][key_of(m)] for n in order], order)
        assert gpu.last_stats == {**gpu.last_stats, "rows": len(order), "host_rows": len(HOST_EDGE)}
    assert rows_of(*gpu.encode_rows([by_name[n]["text"] for n in order], 2)) == [[bos, eos]] * len(order)
    # n = 0
    ptr, out = gpu.encode_rows([])
    assert ptr.tolist() == [0] and out.numel() == 0 and ptr.is_cuda
    assert tuple(gpu([], padding=True, max_length=8)["input_ids"].shape) == (0, 0)


def test_tie_vocabulary():
    """Paths with exactly equal scores: the strict > in start order decides, as in the library's recorded ids."""
    from snx.unigram import UnigramTokenizer
    v = load_variants()["tie"]
    spec = with_vocab(fixture_spec(), [tuple(p) for p in v["pieces"]])
    gpu, cpu = UnigramTokenizer(spec, device="cuda"), UnigramTokenizer(spec, device="cpu")
    texts = [c["text"] for c in v["cases"]]
    assert_rows(rows_of(*gpu.encode_rows(texts)), [c["ids"] for c in v["cases"]], texts)
    assert gpu.last_stats["host_rows"] == 0
    rng = random.Random(12)
    more = [tie_text(rng, 60) for _ in range(2000)]
    assert_rows(rows_of(*gpu.encode_rows(more)), [cpu.host_row(t) for t in more], more)
    # a literal U+2581 (at the start, in the middle, doubled) reaches the pre-tokenizer only past the charsmap
    raw = load_variants()["tie_normalized"]["cases"]
    assert [c["text"] for c in raw] == texts and sum(META in t for t in texts) > 100
    assert_rows(rows_of(*gpu.encode_rows(texts, normalized=True)), [c["ids"] for c in raw], texts)
    assert_rows(rows_of(*gpu.encode_rows(more, 8, normalized=True)), [cpu.host_row(t, 8, normalized=True) for t in more], more)
    fixed = [META + "ab", "ab" + META + "ba", META + META + "ab a" + META + META, META, "a " + META + " " + META + "b"]
    assert_rows(rows_of(*gpu.encode_rows(fixed, normalized=True)), [cpu.host_row(t, None, True) for t in fixed], fixed)


def test_collisions_never_decide_an_id(cpu, pieces):
    """The smallest table the entries fit: 98 % full, probe chains of hundreds of slots."""
    from snx.unigram import UnigramTokenizer
    size = 1
    while size < len(cpu._entries):
        size <<= 1
    assert len(cpu._entries) > 0.95 * size
    small = UnigramTokenizer(fixture_spec(), device="cuda", table_size=size)
    rng = random.Random(99)
    texts = [plain_text(rng, pieces, 120) for _ in range(500)]
    assert_rows(rows_of(*small.encode_rows(texts)), [cpu.host_row(t) for t in texts], texts)
    assert small.last_stats["host_rows"] == 0


def test_long_rows(gpu, cpu, pieces):
    """4,096 normalized code points is the last row of the LDS form; 4,097, 5,005 and 20,000 take the workspace; 513 is the
    first row of the larger LDS form.  One long row is a single word, one grows under the charsmap."""
    rng = random.Random(77)
    long_text = " ".join(rng.choice(pieces) for _ in range(8000))[:19999] + "x"       # pieces are normalized text already
    word = "".join(rng.choice(pieces) for _ in range(3000)).replace(META, "")[:5005]
    grown = chr(0x321C) * 1365 + "ab"                       # 1,367 code points that normalize to 4,097
    edge = "ab " * 1365 + "c"
    texts = ["hello world", long_text, "", "검색 엔진", word, edge, grown, "x" * 512, "y" * 513, "z" * 4096, "끝"]
    norm = [len(cpu.normalize(t)) for t in texts]
    assert norm[1] == 20000 and norm[4] == 5005 and norm[5] == 4096 and norm[6] == 4097 and norm[9] == 4096
    assert " " not in word and not any(gpu._needs_host(t) for t in texts)
    for m in (None, 64):
        got = rows_of(*gpu.encode_rows(texts, m))
        assert_rows(got, [cpu.host_row(t, m) for t in texts], [t[:20] for t in texts])
    assert gpu.last_stats["host_rows"] == 0


def test_host_rows_are_counted(gpu, cpu, pieces):
    rng = random.Random(5)
    texts = [plain_text(rng, pieces, 60) for _ in range(1000)]
    got = rows_of(*gpu.encode_rows(texts, 64))
    assert gpu.last_stats["host_rows"] == 0 and gpu.last_stats["rows"] == 1000
    assert_rows(got, [cpu.host_row(t, 64) for t in texts], texts)
    mixed = list(texts[:20])
    mixed[3] = "cafe" + chr(0x301) + " x"                    # a combining mark
    mixed[7] = chr(0x1112) + chr(0x1161) + chr(0x11AB)       # conjoining jamo
    mixed[8] = "a <mask> b"
    mixed[15] = "<s>"
    got = rows_of(*gpu.encode_rows(mixed, 64))
    assert gpu.last_stats == {**gpu.last_stats, "rows": 20, "host_rows": 4}
    assert_rows(got, [cpu.host_row(t, 64) for t in mixed], mixed)
    assert gpu.mask_token_id in got[8] and got[15] == [0, 0, 2]


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
    assert want[0] == gpu.bos_token_id and one["input_ids"][0].tolist() == want


def _tiny_teacher(vocab_size: int):
    from snx.teacher import TeacherConfig, random_state_dict
    cfg = TeacherConfig(vocab_size=vocab_size, hidden_size=256, intermediate_size=512, num_hidden_layers=2,
                        num_attention_heads=4, max_position_embeddings=140, type_vocab_size=1, pad_token_id=1,
                        layer_norm_eps=1e-5)
    return cfg, random_state_dict(cfg, 24)


def _teacher_texts(pieces):
    rng = random.Random(31)
    texts = [plain_text(rng, pieces, rng.choice((5, 30, 120, 400))) for _ in range(40)]
    return texts + ["", "e" + chr(0x301) + "cole <mask>", texts[3], "x"]


@pytest.mark.parametrize("precision", ("bf16", "fp32"))
def test_teacher_takes_the_csr_and_returns_the_same_bits(gpu, cpu, pieces, precision):
    from snx.teacher import TeacherEncoder
    cfg, sd = _tiny_teacher(len(gpu))
    enc = TeacherEncoder(cfg, sd, device="cuda:0", precision=precision)
    texts = _teacher_texts(pieces)
    assert enc._on_my_gpu(gpu) and not enc._on_my_gpu(cpu)
    lens = [len(cpu.host_row(t, 64)) for t in texts]
    assert min(lens) == 2 and max(lens) == 64 and sum(lens) > 5 * 150       # several batches, a cut row, an empty row
    for kw in (dict(batch_tokens=150), dict(batch_tokens=150, batch_size=7), dict()):
        a = enc.encode(texts, gpu, max_length=64, **kw)
        b = enc.encode(texts, cpu, max_length=64, **kw)
        assert a.is_cuda and tuple(a.shape) == (len(texts), 256) and bool(torch.isfinite(a).all())
        assert torch.equal(a, b), kw
    assert gpu.last_stats["host_rows"] == 1
    assert torch.equal(a[3], a[42]) and not torch.equal(a[3], a[4])
    # the checks of the padded entry hold on the CSR too
    small = TeacherEncoder(*_tiny_teacher(100), device="cuda:0", precision=precision)
    with pytest.raises(ValueError, match="input_ids must lie in"):
        small.encode(texts, gpu, max_length=64)
    with pytest.raises(ValueError, match="max_position_embeddings"):
        enc.encode(["a " * 300], gpu, max_length=300)


def test_teacher_scores_encode_writes_the_same_bytes(tmp_path, gpu, pieces):
    from src.train.cli import teacher_scores
    cfg, sd = _tiny_teacher(len(gpu))
    model = tmp_path / "m"
    os.makedirs(model)
    with open(model / "config.json", "w") as f:
        json.dump({"model_type": "xlm-roberta", "hidden_act": "gelu", **{k: getattr(cfg, k) for k in cfg.__dataclass_fields__}}, f)
    torch.save(sd, model / "pytorch_model.bin")
    texts = _teacher_texts(pieces)
    with open(tmp_path / "train_000.jsonl", "w", encoding="utf-8") as f:
        for i in range(0, len(texts) - 1, 2):
            f.write(json.dumps({"query": texts[i], "positive": texts[i + 1]}, ensure_ascii=False) + "\n")
    outs = {}
    for kind in ("gpu", "unigram"):
        out = tmp_path / kind
        n = teacher_scores.main(["encode", "--model-dir", str(model), "--input-pattern", str(tmp_path / "train_*.jsonl"),
                                 "--output-dir", str(out), "--max-length", "64", "--batch-tokens", "150", "--device", "cuda:0",
                                 "--tokenizer", f"{kind}:{fixture_dir()}"])
        assert n[0] == n[1] >= 30
        outs[kind] = open(out / "embeddings.npy", "rb").read()
    assert len(outs["gpu"]) > 40 * 256 * 4 and outs["gpu"] == outs["unigram"]
