"""CPU checks of the WordPiece tokenizer (snx/wordpiece.py): the host restatement against the `tokenizers` library's
recorded output (tests/golden/g23_tokenizer, tools/make_golden_tokenizer.py) and, where the library imports, against the
library itself; the class table; what the loader refuses; the factory; the fork guard.  No GPU, no transformers."""
import copy
import json
import os
import random
import sys
import types

import pytest
import torch

from tests.wordpiece_reference import (MAX_LENGTHS, key_of, load_cases, random_text, synthetic_spec,
                                       vocabulary_pieces, fixture_dir)


@pytest.fixture(scope="module")
def tok():
    from snx.wordpiece import WordPieceTokenizer
    return WordPieceTokenizer.from_pretrained(fixture_dir(), device="cpu")


@pytest.fixture(scope="module")
def cases():
    return load_cases()


@pytest.mark.parametrize("max_length", MAX_LENGTHS, ids=key_of)
def test_host_restatement_equals_every_golden_row(tok, cases, max_length):
    assert len(cases) >= 300
    for c in cases:
        assert tok.host_row(c["text"], max_length) == c["ids"][key_of(max_length)], (c["name"], max_length)


def test_host_restatement_equals_the_library_on_random_strings(tok):
    tokenizers = pytest.importorskip("tokenizers")
    lib = tokenizers.Tokenizer.from_file(os.path.join(fixture_dir(), "tokenizer.json"))
    lib.no_truncation()
    rng = random.Random(20000)
    pieces = vocabulary_pieces()
    texts = [random_text(rng, pieces, 48) for _ in range(20000)]
    for s in range(0, len(texts), 2000):
        for text, enc in zip(texts[s:s + 2000], lib.encode_batch(texts[s:s + 2000])):
            assert tok.host_row(text) == enc.ids, repr(text)


def test_class_table_whitespace_is_exactly_the_listed_set():
    from snx.wordpiece import PUNCT, SPACE, WHITE_SPACE, class_table
    t = class_table()
    assert t.shape == (0x110000,) and str(t.dtype) == "uint8"
    listed = {0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x20, 0x85, 0xA0, 0x1680, 0x2000, 0x2001, 0x2002, 0x2003, 0x2004, 0x2005,
              0x2006, 0x2007, 0x2008, 0x2009, 0x200A, 0x2028, 0x2029, 0x202F, 0x205F, 0x3000}
    assert set(WHITE_SPACE) == listed
    assert {c for c in range(0x110000) if t[c] == SPACE} == listed
    for c in (0x200B, 0x1C, 0x1D, 0x1E, 0x1F):
        assert t[c] == 0, hex(c)
    for ch in "$+<=>^`|~!\"#%&'()*,-./:;?@[\\]_{}":
        assert t[ord(ch)] == PUNCT, ch
    for ch in "azAZ09가漢あ":
        assert t[ord(ch)] == 0, ch
    for ch in "、—」…。「":
        assert t[ord(ch)] == PUNCT, ch


def _spec():
    with open(os.path.join(fixture_dir(), "tokenizer.json"), encoding="utf-8") as f:
        return json.load(f)


@pytest.mark.parametrize("name,edit,field", [
    ("bert_normalizer", lambda s: s.update(normalizer={"type": "BertNormalizer", "clean_text": True, "lowercase": False,
                                                        "handle_chinese_chars": True, "strip_accents": None}), "normalizer"),
    ("lowercase", lambda s: s.update(normalizer={"type": "BertNormalizer", "lowercase": True}), "normalizer.lowercase"),
    ("metaspace", lambda s: s.update(pre_tokenizer={"type": "Metaspace", "replacement": "▁"}), "pre_tokenizer"),
    ("bpe", lambda s: s["model"].update(type="BPE"), "model.type"),
    ("roberta_post", lambda s: s.update(post_processor={"type": "RobertaProcessing"}), "post_processor"),
    ("pair_template", lambda s: s["post_processor"].update(single=s["post_processor"]["pair"]), "post_processor.single"),
    ("two_pretokenizers", lambda s: s["pre_tokenizer"]["pretokenizers"].append({"type": "Whitespace"}), "pre_tokenizer"),
    ("stripping_added_token", lambda s: s["added_tokens"][4].update(lstrip=True), "added_tokens"),
    ("long_words", lambda s: s["model"].update(max_input_chars_per_word=1000), "model.max_input_chars_per_word"),
])
def test_loader_refuses_other_pipelines_and_names_the_field(name, edit, field):
    from snx.wordpiece import WordPieceTokenizer
    spec = copy.deepcopy(_spec())
    edit(spec)
    with pytest.raises(ValueError) as e:
        WordPieceTokenizer(spec, device="cpu")
    assert f"tokenizer.json: {field}:" in str(e.value), str(e.value)


def test_loader_refuses_a_directory_with_only_vocab_txt(tmp_path):
    from snx.wordpiece import WordPieceTokenizer
    (tmp_path / "vocab.txt").write_text("<s>\n</s>\n<unk>\na\n", encoding="utf-8")
    with pytest.raises(ValueError, match="tokenizer.json"):
        WordPieceTokenizer.from_pretrained(str(tmp_path), device="cpu")


def test_loader_accepts_no_normalizer_and_a_bare_pre_tokenizer(tok):
    from snx.wordpiece import WordPieceTokenizer
    spec = copy.deepcopy(_spec())
    spec["normalizer"] = None
    spec["pre_tokenizer"] = {"type": "BertPreTokenizer"}
    t = WordPieceTokenizer(spec, device="cpu")
    assert t.host_row("hello world") == tok.host_row("hello world")
    assert t.host_row("e\u0301") != tok.host_row("e\u0301")      # nothing composes the accent


def test_factory_dispatch(monkeypatch, tmp_path):
    from snx.wordpiece import WordPieceTokenizer
    from src.train.data.collator import HashTokenizer, create_tokenizer
    cpu = create_tokenizer("wordpiece:" + fixture_dir())
    gpu = create_tokenizer("gpu:" + fixture_dir())        # built without touching a GPU: the tables are uploaded on first use
    assert type(cpu) is WordPieceTokenizer and type(gpu) is WordPieceTokenizer
    assert cpu.device.type == "cpu" and gpu.device.type == "cuda"
    # existing names keep their meaning
    assert isinstance(create_tokenizer("hash:1000"), HashTokenizer)
    HashTokenizer(777).save_pretrained(str(tmp_path / "h"))
    assert create_tokenizer(str(tmp_path / "h")).vocab_size == 777
    seen = []
    fake = types.ModuleType("transformers")
    fake.AutoTokenizer = types.SimpleNamespace(from_pretrained=lambda name: seen.append(name) or "auto")
    monkeypatch.setitem(sys.modules, "transformers", fake)
    assert create_tokenizer(fixture_dir()) == "auto" and seen == [fixture_dir()]      # a bare directory: AutoTokenizer


def test_device_call_from_another_process_raises(monkeypatch):
    import snx.wordpiece as W
    t = W.WordPieceTokenizer.from_pretrained(fixture_dir(), device="cuda")
    real = os.getpid()
    monkeypatch.setattr(W.os, "getpid", lambda: real + 1)
    for call in (lambda: t(["hello"]), lambda: t.encode("hello"), lambda: t.encode_rows(["hello"])):
        with pytest.raises(RuntimeError) as e:
            call()
        assert "num_workers=0" in str(e.value) and 'device="cpu"' in str(e.value)
    cpu = W.WordPieceTokenizer.from_pretrained(fixture_dir(), device="cpu")     # the host form has nothing to guard
    assert cpu.encode("hello")[0] == cpu.bos_token_id


def test_call_surface_on_the_host(tok, cases, tmp_path):
    assert (tok.vocab_size, len(tok)) == (49999, 50000)
    assert (tok.bos_token_id, tok.eos_token_id, tok.unk_token_id, tok.pad_token_id) == (0, 1, 2, 49999)
    assert (tok.sep_token_id, tok.mask_token_id, tok.cls_token_id) == (3, 4, 5)
    texts = [c["text"] for c in cases[:60]]
    out = tok(texts, padding=True, truncation=True, max_length=8, return_tensors="pt")
    ids, mask = out["input_ids"], out["attention_mask"]
    want = [c["ids"]["8"] for c in cases[:60]]
    L = max(len(w) for w in want)
    assert ids.shape == mask.shape == (60, L) and ids.dtype == mask.dtype == torch.long
    for r, w in enumerate(want):
        assert ids[r].tolist() == w + [tok.pad_token_id] * (L - len(w))
        assert mask[r].tolist() == [1] * len(w) + [0] * (L - len(w))
    lists = tok(texts, padding=False, truncation=False)
    assert lists["input_ids"] == [c["ids"]["none"] for c in cases[:60]]
    assert [len(m) for m in lists["attention_mask"]] == [len(w) for w in lists["input_ids"]]
    one = tok("hello world", max_length=64)
    assert one["input_ids"].shape[0] == 1 and one["input_ids"][0].tolist() == tok.encode("hello world")
    assert tok.encode("hello world", add_special_tokens=False) == tok.encode("hello world")[1:-1]
    ptr, flat = tok.encode_rows(texts, max_length=64)
    assert ptr.tolist()[-1] == flat.numel() and flat[ptr[3]:ptr[4]].tolist() == cases[3]["ids"]["64"]
    assert tok.convert_ids_to_tokens([0, 1, 2, 49999]) == ["<s>", "<\\s>", "<unk>", "<pad>"]
    assert tok.decode(tok.encode("hello world", add_special_tokens=False)) == "hello world"
    with pytest.raises(ValueError, match="max_length"):
        tok(["a"], max_length=1)
    tok.save_pretrained(str(tmp_path / "saved"))
    assert sorted(os.listdir(tmp_path / "saved")) == ["special_tokens_map.json", "tokenizer.json", "tokenizer_config.json"]
    from snx.wordpiece import WordPieceTokenizer
    again = WordPieceTokenizer.from_pretrained(str(tmp_path / "saved"), device="cpu")
    assert again.host_row(cases[33]["text"]) == cases[33]["ids"]["none"]


def test_hash_table_holds_every_reachable_entry_once():
    """The table the device probes, rebuilt here: every entry is found from its home slot by linear probing, and a
    synthetic vocabulary with both forms of a key keeps them apart."""
    from snx.wordpiece import WordPieceTokenizer, entry_hash
    vocab = {"<s>": 0, "</s>": 1, "<unk>": 2, "ab": 3, "##ab": 4, "a": 5, "##b": 6, "!": 7}
    t = WordPieceTokenizer(synthetic_spec(vocab), device="cpu", table_size=8)
    assert sorted(t._entries) == [(0, "!", 7), (0, "a", 5), (0, "ab", 3), (1, "ab", 4), (1, "b", 6)]
    assert t.host_row("ab abab a!b") == [0, 3, 3, 4, 5, 7, 2, 1]
    assert entry_hash(0, [97, 98]) != entry_hash(1, [97, 98])
    with pytest.raises(ValueError, match="table_size"):
        WordPieceTokenizer(synthetic_spec(vocab), device="cpu", table_size=4)
    with pytest.raises(ValueError, match="table_size"):
        WordPieceTokenizer(synthetic_spec(vocab), device="cpu", table_size=12)


def test_device_tables_find_every_entry_by_the_probe_the_header_states(tok):
    """The device's lookup restated over the uploaded arrays: home slot from the hash, linear probing, stored code points
    compared; and a candidate's hash from the word's prefix hashes equals the hash of the candidate alone."""
    from snx.wordpiece import entry_hash
    tb, mask = tok.device_tables(), tok.table_size - 1
    assert tok.table_size >= 2 * len(tok._entries) and all(v.dtype.name == "int32" for v in tb.values())

    def lookup(cont, cps):
        s = entry_hash(cont, cps) & mask
        for _ in range(tok.table_size):
            e = int(tb["slots"][s])
            if e < 0:
                return -1
            b, en = int(tb["ent_ptr"][e]), int(tb["ent_ptr"][e + 1])
            if en - b == len(cps) and int(tb["ent_cont"][e]) == cont and tb["ent_cps"][b:en].tolist() == cps:
                return int(tb["ent_id"][e])
            s = (s + 1) & mask
        return -1

    for cont, key, tid in tok._entries[::5]:
        assert lookup(cont, [ord(c) for c in key]) == tid, (cont, key)
    assert lookup(0, [0x10FFFF, 1, 2]) == -1 and lookup(1, [ord("q")] * 15) == -1
    B, M = 0x9E3779B1, 0xFFFFFFFF
    word = [ord(c) for c in "tokenization\u200b\uac00\ub098\ub2e4"]
    hx, h = [], 0
    for c in word:
        h = (h * B + c + 1) & M
        hx.append(h)
    for st in range(len(word)):
        for en in range(st + 1, len(word) + 1):
            via_prefix = (hx[en - 1] - (hx[st - 1] if st else 0) * pow(B, en - st, 1 << 32)) & M
            direct = 0
            for c in word[st:en]:
                direct = (direct * B + c + 1) & M
            assert via_prefix == direct


def test_shapes_are_checked_on_the_host_before_any_launch():
    import ctypes as C
    from snx import fn
    one = C.c_void_p(16)
    pieces = fn("snx_wp_pieces")

    def call(n=1, longest=8, n_slots=8, n_entries=4, max_entry=15, max_word=100, ptr=one, cls=one, ws=None, ws_bytes=0):
        return pieces(ptr, one, n, longest, cls, one, n_slots, one, one, one, one, n_entries, max_entry, max_word, 2, -1, one,
                      one, ws, ws_bytes, None)
    assert call(n=-1) == -2 and call(longest=-1) == -2 and call(longest=2 ** 31) == -2
    assert call(n_slots=12) == -2 and call(n_slots=0) == -2 and call(n_entries=9) == -2          # a power of two >= entries
    assert call(max_entry=0) == -2 and call(max_entry=101) == -2 and call(max_word=129, max_entry=129) == -2
    assert call(ptr=None) == -3 and call(cls=None) == -3
    assert call(longest=5000) == -3                                                              # a long row needs the workspace
    need = fn("snx_wp_workspace_bytes")(5000)
    assert need == 64 * 5000 * 4 and fn("snx_wp_workspace_bytes")(4096) == 0 and fn("snx_wp_workspace_bytes")(-1) == 0
    assert call(longest=5000, ws=one, ws_bytes=need - 1) == -3
    assert call(n=0, ptr=None) == 0
    assert fn("snx_wp_fill")(one, one, -1, one, 0, 1, one, None) == -2 and fn("snx_wp_fill")(one, one, 1, None, 0, 1, one, None) == -3
    assert fn("snx_wp_pad")(one, one, 1, -1, 0, one, one, None) == -2 and fn("snx_wp_pad")(one, one, 1, 4, 0, None, one, None) == -3
    assert fn("snx_wp_pad")(None, None, 0, 4, 0, None, None, None) == 0
