"""CPU checks of the text kernels' shared host front: the one ``code_point_csr`` (snx/_text.py) through the four names it
is reached by, and the tokenizer base (snx/_tokenizer.py) under both models.  No GPU."""
import os

import numpy as np
import pytest
import torch

from tests import unigram_reference, wordpiece_reference

EDGE_BATCHES = [
    [],
    [""],
    ["", "a", ""],
    ["\U0001F600", "a\U00010348b"],                             # astral: one code point each
    ["İ", "İstanbul İ"],                                        # lower() grows it to two code points
    ["　 wide 　", "\x85next line\x85", "　", "\x85"],
    ["a\0b", "\0", "\0\0 x"],
    ["", "가나다", "　\0İ\U0001F600\x85", ""],
]


def expected(texts):
    cps = np.frombuffer("".join(texts).encode("utf-32-le"), "<u4")
    ptr = np.concatenate([[0], np.cumsum([len(t) for t in texts])]).astype(np.int64)
    return ptr, cps


def as_it_is():
    from snx import _text, textprep, wordpiece
    return {"_text.code_point_csr": _text.code_point_csr, "textprep.code_point_csr": textprep.code_point_csr,
            "wordpiece.code_point_rows": wordpiece.code_point_rows}


def every_name():
    from snx import minhash
    return dict(as_it_is(), **{"minhash.code_point_csr": minhash.code_point_csr})


@pytest.mark.parametrize("texts", EDGE_BATCHES, ids=[str(i) for i in range(len(EDGE_BATCHES))])
def test_code_point_csr_of_the_edge_texts_through_every_name(texts):
    from snx import _text, minhash
    want_ptr, want_cps = expected(texts)
    for name, f in as_it_is().items():
        ptr, cps = f(texts)
        assert ptr.dtype == np.int64 and cps.dtype == np.int32, name
        assert ptr.tolist() == want_ptr.tolist() and cps.tolist() == want_cps.tolist(), name
        assert ptr.shape == (len(texts) + 1,) and cps.shape == (int(want_ptr[-1]),), name
    low = [t.lower().strip() for t in texts]
    ptr, cps = minhash.code_point_csr(texts)
    l_ptr, l_cps = _text.code_point_csr(low)
    assert ptr.dtype == np.int64 and cps.dtype == np.int32
    assert ptr.tolist() == l_ptr.tolist() == expected(low)[0].tolist()
    assert cps.tolist() == l_cps.tolist() == expected(low)[1].tolist()


def test_lower_and_strip_change_the_rows_minhash_sees():
    from snx import minhash
    ptr, cps = minhash.code_point_csr(["İ", "　 A \x85", "\0 "])
    assert ptr.tolist() == [0, 2, 3, 4] and cps.tolist() == [0x69, 0x307, 0x61, 0]


def test_a_lone_surrogate_is_reported_with_its_index_through_every_name():
    from snx._text import LoneSurrogateError
    from snx import textprep
    assert textprep.LoneSurrogateError is LoneSurrogateError and issubclass(LoneSurrogateError, ValueError)
    texts = ["ok", "가", " BAD \ud800 text ", "\udfff"]
    for name, f in every_name().items():
        with pytest.raises(LoneSurrogateError, match="lone surrogate") as e:
            f(texts, "caller")
        assert e.value.index == 2, name
        assert str(e.value).startswith("caller: ") and "text 2" in str(e.value), name
    # MinHash finds it in what lower and strip leave: a surrogate at the edge is not white space and stays
    from snx import minhash
    with pytest.raises(LoneSurrogateError) as e:
        minhash.code_point_csr(["  ", "A\udc00  "], "caller")
    assert e.value.index == 1


def test_a_text_that_is_no_string_is_refused_through_every_name():
    for name, f in every_name().items():
        for bad in (["a", 3], ["a", b"b"], [None]):
            with pytest.raises(ValueError, match="caller: texts must be strings"):
                f(bad, "caller")


def test_tfidf_rows_come_from_the_same_front():
    from snx._text import LoneSurrogateError
    from snx.retrieval import tfidf
    assert tfidf.code_point_csr.__module__ == "snx._text"
    ptr, cps = tfidf.word_rows(["  Ab\t\tC \n", "İx"])
    assert ptr.tolist() == [0, 4, 7] and cps.tolist() == [ord(c) for c in "ab c"] + [0x69, 0x307, ord("x")]
    with pytest.raises(LoneSurrogateError) as e:
        tfidf.word_rows(["a", "b \udc00"], "caller")
    assert e.value.index == 1


def test_csr_to_device_checks_its_arguments_before_it_touches_a_gpu():
    from snx._text import code_point_csr, csr_to_device
    ptr, cps = code_point_csr(["ab", ""])
    for trusted in (False, True):
        with pytest.raises(ValueError, match="caller: rows are ptr int64"):
            csr_to_device(ptr.astype(np.int32), cps, "cuda", "caller", trusted=trusted)
        with pytest.raises(ValueError, match="caller: rows are ptr int64"):
            csr_to_device(ptr, cps.astype(np.int64), "cuda", "caller", trusted=trusted)
        with pytest.raises(ValueError, match="caller: runs on a GPU"):
            csr_to_device(ptr, cps, "cpu", "caller", trusted=trusted)


# ---------------------------------------------------------------------------------------------------- the tokenizer base
def test_both_tokenizers_derive_from_the_base_and_not_from_each_other():
    from snx._tokenizer import RowTokenizer
    from snx.unigram import UnigramTokenizer
    from snx.wordpiece import WordPieceTokenizer
    assert issubclass(WordPieceTokenizer, RowTokenizer) and issubclass(UnigramTokenizer, RowTokenizer)
    assert not issubclass(UnigramTokenizer, WordPieceTokenizer) and not issubclass(WordPieceTokenizer, UnigramTokenizer)
    for cls in (WordPieceTokenizer, UnigramTokenizer):                  # one copy of what the base holds
        for name in ("__init__", "from_pretrained", "_parse_template", "_roles", "host_pieces", "_guard", "_device_state",
                     "_texts", "_max_length", "_encode_rows", "_finish_rows", "__call__", "encode", "convert_ids_to_tokens",
                     "get_vocab", "save_pretrained"):
            assert name not in vars(cls), (cls.__name__, name)
    from snx import wordpiece
    for name in ("entry_hash", "WHITE_SPACE", "class_table", "PUNCT", "SPACE", "_refuse"):
        assert hasattr(wordpiece, name), name


def test_the_fork_guard_names_the_class_and_its_factory_prefix(monkeypatch):
    from snx.unigram import UnigramTokenizer
    from snx.wordpiece import WordPieceTokenizer
    made = [(WordPieceTokenizer.from_pretrained(wordpiece_reference.fixture_dir(), device="cuda"), "wordpiece"),
            (UnigramTokenizer.from_pretrained(unigram_reference.fixture_dir(), device="cuda"), "unigram")]
    real = os.getpid()
    monkeypatch.setattr(os, "getpid", lambda: real + 1)
    for tok, prefix in made:
        with pytest.raises(RuntimeError) as e:
            tok.encode_rows(["hello"])
        assert str(e.value).startswith(type(tok).__name__ + ": this tokenizer was created in another process")
        assert f'create_tokenizer("{prefix}:DIR")' in str(e.value) and "num_workers=0" in str(e.value)


@pytest.fixture(scope="module")
def wp():
    from snx.wordpiece import WordPieceTokenizer
    return WordPieceTokenizer.from_pretrained(wordpiece_reference.fixture_dir(), device="cpu")


@pytest.fixture(scope="module")
def ug():
    from snx.unigram import UnigramTokenizer
    return UnigramTokenizer.from_pretrained(unigram_reference.fixture_dir(), device="cpu")


def check_padded(tok, texts, want):
    out = tok(texts, padding=True, truncation=True, max_length=8, return_tensors="pt")
    ids, mask = out["input_ids"], out["attention_mask"]
    L = max(len(w) for w in want)
    assert ids.shape == mask.shape == (len(want), L) and ids.dtype == mask.dtype == torch.long
    for r, w in enumerate(want):
        assert ids[r].tolist() == w + [tok.pad_token_id] * (L - len(w))
        assert mask[r].tolist() == [1] * len(w) + [0] * (L - len(w))


def test_wordpiece_call_surface_on_the_host(wp, tmp_path):
    from snx.wordpiece import WordPieceTokenizer
    tok, cases = wp, wordpiece_reference.load_cases()
    assert (tok.vocab_size, len(tok)) == (49999, 50000)
    assert (tok.bos_token_id, tok.eos_token_id, tok.unk_token_id, tok.pad_token_id) == (0, 1, 2, 49999)
    assert (tok.sep_token_id, tok.mask_token_id, tok.cls_token_id) == (3, 4, 5)
    texts = [c["text"] for c in cases[:60]]
    check_padded(tok, texts, [c["ids"]["8"] for c in cases[:60]])
    lists = tok(texts, padding=False, truncation=False)
    assert lists["input_ids"] == [c["ids"]["none"] for c in cases[:60]]
    assert [len(m) for m in lists["attention_mask"]] == [len(w) for w in lists["input_ids"]]
    one = tok("hello world", max_length=64)
    assert one["input_ids"].shape[0] == 1 and one["input_ids"][0].tolist() == tok.encode("hello world")
    assert tok.encode("hello world", add_special_tokens=False) == tok.encode("hello world")[1:-1]
    ptr, flat = tok.encode_rows(texts, max_length=64)
    assert ptr.tolist()[-1] == flat.numel() and flat[ptr[3]:ptr[4]].tolist() == cases[3]["ids"]["64"]
    assert tok.last_stats["rows"] == tok.last_stats["host_rows"] == 60
    assert tok.convert_ids_to_tokens([0, 1, 2, 49999]) == ["<s>", "<\\s>", "<unk>", "<pad>"]
    assert tok.decode(tok.encode("hello world", add_special_tokens=False)) == "hello world"
    assert tok.get_vocab()["<pad>"] == 49999 and len(tok.get_vocab()) == 50000
    with pytest.raises(ValueError, match="WordPieceTokenizer: max_length"):
        tok(["a"], max_length=1)
    tok.save_pretrained(str(tmp_path / "saved"))
    assert sorted(os.listdir(tmp_path / "saved")) == ["special_tokens_map.json", "tokenizer.json", "tokenizer_config.json"]
    again = WordPieceTokenizer.from_pretrained(str(tmp_path / "saved"), device="cpu")
    assert again.host_row(cases[33]["text"]) == cases[33]["ids"]["none"]
    assert again.get_vocab() == tok.get_vocab()


def test_unigram_call_surface_on_the_host(ug, tmp_path):
    from snx.unigram import UnigramTokenizer
    tok, cases = ug, unigram_reference.load_cases()
    n = len(unigram_reference.fixture_spec()["model"]["vocab"])
    assert (tok.vocab_size, len(tok)) == (n, n)
    assert (tok.bos_token_id, tok.pad_token_id, tok.eos_token_id, tok.unk_token_id, tok.mask_token_id) == (0, 1, 2, 3, n - 1)
    assert (tok.cls_token_id, tok.sep_token_id) == (0, 2)
    texts = [c["text"] for c in cases[:60]]
    check_padded(tok, texts, [c["ids"]["8"] for c in cases[:60]])
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
    again = UnigramTokenizer.from_pretrained(str(tmp_path / "saved"), device="cpu")
    assert again.host_row(cases[44]["text"]) == cases[44]["ids"]["none"]
    assert again.get_vocab() == tok.get_vocab()
