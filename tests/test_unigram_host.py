"""CPU checks of the Unigram tokenizer (snx/unigram.py): the host restatement against the `tokenizers` library's recorded
output (tests/golden/g24_unigram, written by tools/make_golden_unigram.py) and, where the library imports, against the
library itself; the charsmap parser; the loader's refusals; the factory.  Every comparison is id for id."""
import random

import pytest

from tests.unigram_reference import (MAX_LENGTHS, META, fixture_dir, fixture_spec, key_of, load_cases, load_variants,
                                     mask_lstrip_spec, old_form_spec, plain_text, random_text, tie_text, vocabulary_pieces,
                                     with_vocab)


@pytest.fixture(scope="module")
def tok():
    from snx.unigram import UnigramTokenizer
    return UnigramTokenizer.from_pretrained(fixture_dir(), device="cpu")


@pytest.fixture(scope="module")
def cases():
    return load_cases()


@pytest.fixture(scope="module")
def variants():
    return load_variants()


@pytest.mark.parametrize("max_length", MAX_LENGTHS, ids=key_of)
def test_restatement_equals_every_golden_row(tok, cases, max_length):
    assert len(cases) >= 340
    for c in cases:
        assert tok.host_row(c["text"], max_length) == c["ids"][key_of(max_length)], c["name"]


def test_charsmap_parser_reproduces_the_normalized_form(tok, cases):
    changed = 0
    for c in cases:
        assert tok.normalize(c["text"]) == c["normalized"], c["name"]
        changed += c["normalized"] != c["text"]
    assert changed > 100
    nmap, pool = tok.charsmap.code_point_map
    # what the issue measured on this charsmap: 5,008 rewritten code points, the longest replacement U+FDFA's 18
    assert int((nmap >= 0).sum()) == 5008 and int((nmap[nmap >= 0] & 31).max()) == 18
    assert nmap[0xFDFA] & 31 == 18 and 0x20 in pool[nmap[0xFDFA] >> 5:(nmap[0xFDFA] >> 5) + 18].tolist()
    assert int(((nmap >= 0) & (nmap & 31 == 0)).sum()) > 0                      # some replacements are empty
    assert tok.charsmap.normalize_plain("Ａ① ㈜") == "A1 (주)"


def test_tie_vocabulary(variants):
    from snx.unigram import UnigramTokenizer
    tie = UnigramTokenizer(with_vocab(fixture_spec(), [tuple(p) for p in variants["tie"]["pieces"]]), device="cpu")
    assert len(variants["tie"]["pieces"]) == 46 and all(s * 2 == int(s * 2) for _, s in variants["tie"]["pieces"])
    assert "c" not in tie.get_vocab()
    for c in variants["tie"]["cases"]:
        assert tie.host_row(c["text"]) == c["ids"], repr(c["text"])
    assert any(tie.unk_token_id in c["ids"] for c in variants["tie"]["cases"])
    # the same rows past the normalizer (the library's ids with the normalizer taken out): a literal U+2581 survives
    raw = variants["tie_normalized"]["cases"]
    assert sum(META in c["text"] for c in raw) > 100
    for c in raw:
        assert tie.host_row(c["text"], normalized=True) == c["ids"], repr(c["text"])
    ptr, ids = tie.encode_rows([c["text"] for c in raw[:50]], normalized=True)
    assert ids.tolist() == [i for c in raw[:50] for i in c["ids"]]


@pytest.mark.parametrize("name,edit", [("old_form", old_form_spec), ("mask_lstrip", mask_lstrip_spec)])
def test_variants_of_the_pipeline(cases, variants, name, edit):
    """The old serialized form gives the new form's ids; lstrip on an added token changes no id under WhitespaceSplit."""
    from snx.unigram import UnigramTokenizer
    t = UnigramTokenizer(edit(fixture_spec()), device="cpu")
    assert len(variants[name]["cases"]) == len(cases)
    for c, base in zip(variants[name]["cases"], cases):
        assert c["text"] == base["text"] and c["ids"] == base["ids"]["none"], base["name"]    # recorded from the library
        assert t.host_row(c["text"]) == c["ids"], base["name"]


def test_restatement_equals_the_library_on_random_strings(tok, variants):
    tokenizers = pytest.importorskip("tokenizers")
    import json
    from snx.unigram import UnigramTokenizer
    lib = tokenizers.Tokenizer.from_file(fixture_dir() + "/tokenizer.json")
    lib.no_truncation()
    rng = random.Random(20000)
    pieces = vocabulary_pieces()
    texts = [random_text(rng, pieces, 60) for _ in range(20000)]
    for t, e in zip(texts, lib.encode_batch(texts)):
        assert tok.host_row(t) == e.ids, repr(t)
    spec = with_vocab(fixture_spec(), [tuple(p) for p in variants["tie"]["pieces"]])
    tie, tie_lib = UnigramTokenizer(spec, device="cpu"), tokenizers.Tokenizer.from_str(json.dumps(spec))
    texts = [tie_text(rng) for _ in range(20000)]
    for t, e in zip(texts, tie_lib.encode_batch(texts)):
        assert tie.host_row(t) == e.ids, repr(t)


def test_rows_without_joining_code_points_normalize_code_point_by_code_point(tok):
    """The device's precondition, on the host: such a row's cluster walk and its code point walk agree."""
    rng = random.Random(7)
    pieces = vocabulary_pieces()
    for _ in range(3000):
        t = plain_text(rng, pieces, 80)
        assert not tok._needs_host(t), repr(t)
        clusters = "".join(tok.charsmap.transform(c.encode("utf-8")) if tok.charsmap.transform(c.encode("utf-8")) is not None
                           else c for c in t)
        assert tok.charsmap.normalize_plain(t) == clusters
    for t in ("e" + chr(0x301), chr(0x1112) + chr(0x1161), "a\r\nb", chr(0x1F1F0) + chr(0x1F1F7), "x" + chr(0x200D) + "y", "a <mask>",
              chr(0x915) + chr(0x94D)):
        assert tok._needs_host(t), repr(t)


def _edits():
    long_piece = META + "x" * 32
    return [
        ("bpe", lambda s: s["model"].update(type="BPE"), "model.type"),
        ("byte_fallback", lambda s: s["model"].update(byte_fallback=True), "model.byte_fallback"),
        ("nfkc", lambda s: s.update(normalizer={"type": "NFKC"}), "normalizer"),
        ("no_normalizer", lambda s: s.update(normalizer=None), "normalizer"),
        ("other_replace", lambda s: s.update(normalizer={"type": "Sequence", "normalizers": [
            s["normalizer"], {"type": "Replace", "pattern": {"String": "a"}, "content": "b"}]}), "normalizer"),
        ("no_whitespace_split", lambda s: s["pre_tokenizer"]["pretokenizers"].pop(0), "pre_tokenizer"),
        ("bare_metaspace", lambda s: s.update(pre_tokenizer=s["pre_tokenizer"]["pretokenizers"][1]), "pre_tokenizer"),
        ("prepend_first", lambda s: s["pre_tokenizer"]["pretokenizers"][1].update(prepend_scheme="first"),
         "pre_tokenizer.prepend_scheme"),
        ("no_split", lambda s: s["pre_tokenizer"]["pretokenizers"][1].update(split=False), "pre_tokenizer.split"),
        ("repeated_piece", lambda s: s["model"]["vocab"].append(list(s["model"]["vocab"][10])), "model.vocab"),
        ("long_piece", lambda s: s["model"]["vocab"].append([long_piece, -5.0]), "model.vocab"),
        ("unk_id", lambda s: s["model"].update(unk_id=None), "model.unk_id"),
        ("normalized_added", lambda s: s["added_tokens"][4].update(normalized=True), "added_tokens[4].normalized"),
        ("single_word_added", lambda s: s["added_tokens"][0].update(single_word=True), "added_tokens[0].single_word"),
        ("roberta_post", lambda s: s.update(post_processor={"type": "RobertaProcessing"}), "post_processor"),
        ("pair_template", lambda s: s["post_processor"].update(single=s["post_processor"]["pair"]), "post_processor.single"),
    ]


@pytest.mark.parametrize("name,edit,field", _edits(), ids=[e[0] for e in _edits()])
def test_loader_refuses_other_pipelines_and_names_the_field(name, edit, field):
    from snx.unigram import UnigramTokenizer
    spec = fixture_spec()
    edit(spec)
    with pytest.raises(ValueError) as e:
        UnigramTokenizer(spec, device="cpu")
    assert f"tokenizer.json: {field}:" in str(e.value), str(e.value)
    if name == "long_piece":
        assert "32" in str(e.value) and "33 code points" in str(e.value)


def test_loader_accepts_a_piece_of_exactly_the_bound():
    from snx.unigram import MAX_PIECE, UnigramTokenizer
    spec = fixture_spec()
    spec["model"]["vocab"].insert(-1, [META + "x" * (MAX_PIECE - 1), -5.0])
    spec["added_tokens"][4]["id"] += 1
    t = UnigramTokenizer(spec, device="cpu")
    assert MAX_PIECE >= 32 and t._max_entry == MAX_PIECE
    assert t.host_pieces("x" * (MAX_PIECE - 1)) == [len(spec["model"]["vocab"]) - 2]


def test_factory_dispatch():
    from snx.unigram import UnigramTokenizer
    from snx.wordpiece import WordPieceTokenizer
    from src.train.data.collator import create_tokenizer
    from tests import wordpiece_reference as W
    cpu = create_tokenizer("unigram:" + fixture_dir())
    gpu = create_tokenizer("gpu:" + fixture_dir())        # built without touching a GPU: the tables are uploaded on first use
    assert type(cpu) is UnigramTokenizer and type(gpu) is UnigramTokenizer
    assert cpu.device.type == "cpu" and gpu.device.type == "cuda"
    assert type(create_tokenizer("wordpiece:" + W.fixture_dir())) is WordPieceTokenizer
    assert type(create_tokenizer("gpu:" + W.fixture_dir())) is WordPieceTokenizer
    with pytest.raises(ValueError, match="tokenizer.json: normalizer"):    # the other loader refuses the file
        create_tokenizer("wordpiece:" + fixture_dir())


def test_device_call_from_another_process_raises(monkeypatch):
    import snx.unigram as U
    t = U.UnigramTokenizer.from_pretrained(fixture_dir(), device="cuda")
    real = U.os.getpid()
    monkeypatch.setattr(U.os, "getpid", lambda: real + 1)
    for call in (lambda: t(["hello"]), lambda: t.encode("hello"), lambda: t.encode_rows(["hello"])):
        with pytest.raises(RuntimeError) as e:
            call()
        assert "num_workers=0" in str(e.value) and "unigram:DIR" in str(e.value)


def test_call_surface_on_the_host(tok, cases, tmp_path):
    import torch
    n = len(fixture_spec()["model"]["vocab"])
    assert (tok.vocab_size, len(tok)) == (n, n)
    assert (tok.bos_token_id, tok.pad_token_id, tok.eos_token_id, tok.unk_token_id, tok.mask_token_id) == (0, 1, 2, 3, n - 1)
    assert (tok.cls_token_id, tok.sep_token_id) == (0, 2)
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
    assert tok.encode("hello world", add_special_tokens=False) == tok.encode("hello world")[1:-1]
    ptr, flat = tok.encode_rows(texts, max_length=64)
    assert ptr.tolist()[-1] == flat.numel() and flat[ptr[5]:ptr[6]].tolist() == cases[5]["ids"]["64"]
    assert tok.last_stats["rows"] == tok.last_stats["host_rows"] == 60
    assert tok.convert_ids_to_tokens([0, 1, 2, 3, n - 1]) == ["<s>", "<pad>", "</s>", "<unk>", "<mask>"]
    assert tok.decode(tok.encode("hello  world", add_special_tokens=False)) == "hello world"
    assert tok.decode(tok.encode("hello world"), skip_special_tokens=True) == "hello world"
    assert tok.get_vocab()["<mask>"] == n - 1
    with pytest.raises(ValueError, match="UnigramTokenizer: max_length"):
        tok(["a"], max_length=1)
    tok.save_pretrained(str(tmp_path / "saved"))
    from snx.unigram import UnigramTokenizer
    again = UnigramTokenizer.from_pretrained(str(tmp_path / "saved"), device="cpu")
    assert again.host_row(cases[44]["text"]) == cases[44]["ids"]["none"]


def test_device_table_holds_every_reachable_piece_once(tok):
    from snx.wordpiece import entry_hash
    tables = tok.device_tables()
    slots, ent_ptr, ent_cps = tables["slots"], tables["ent_ptr"], tables["ent_cps"]
    assert sorted(slots[slots >= 0].tolist()) == list(range(len(tok._entries)))
    assert tables["ent_score"].dtype.name == "float64" and tables["ent_score"].shape == (len(tok._entries),)
    mask = tok.table_size - 1
    for e, (_, key, tid) in enumerate(tok._entries):
        assert META not in key[1:] and " " not in key
        s = entry_hash(0, [ord(ch) for ch in key]) & mask
        while slots[s] != e:
            assert slots[s] >= 0
            s = (s + 1) & mask
        assert "".join(map(chr, ent_cps[ent_ptr[e]:ent_ptr[e + 1]])) == key and tables["ent_id"][e] == tid
        assert tables["ent_score"][e] == tok._scores[tid]
    assert tok._unk_score == min(tok._scores) - 10.0
