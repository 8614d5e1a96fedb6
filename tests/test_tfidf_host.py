"""Host checks of the character n-gram TF-IDF step (include/snx.h "Character n-gram TF-IDF"): the restatement of the
contract (tests/tfidf_reference.py) against what scikit-learn and the reference's miner produced (tests/golden/g17_tfidf,
written by tools/make_golden_tfidf.py; nothing of either is read at test time), the host half of snx.retrieval.tfidf, the
miner's host logic on the numpy stand-in, and the CLI's flags.  No GPU."""
import inspect
import json
import os
import shutil

import numpy as np
import pytest
import torch

from tests import tfidf_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G17 = os.path.join(ROOT, "tests", "golden", "g17_tfidf")


@pytest.fixture(scope="module")
def g17():
    return R.load_g17(G17)


@pytest.fixture(scope="module")
def model(g17):
    return R.fit(g17["corpus"], (2, 3), g17["max_features"])


def _ulps32(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Distance in fp32 ulps of positive fp32 values."""
    return np.abs(a.astype(np.float32).view(np.int32).astype(np.int64) - b.astype(np.float32).view(np.int32).astype(np.int64))


# ------------------------------------------------------------------------------------------------ the analyzer and the key
def test_analyzer_hand_cases():
    assert R.analyze("a") == [" a", "a ", " a "]                        # L == 3: the trigram is the whole padded word
    assert R.analyze("ab cd") == [" a", "ab", "b ", " ab", "ab ", " c", "cd", "d ", " cd", "cd "]   # none across the space
    assert R.analyze("aaaa") == [" a", "aa", "aa", "aa", "a ", " aa", "aaa", "aaa", "aa "]
    assert R.analyze("") == [] and R.analyze(" \t\n  ") == []
    assert R.analyze("A\tb", (1, 1)) == [" ", "a", " ", " ", "b", " "]  # a padded word holds its own two blanks
    assert R.analyze("a", (3, 3)) == [" a "] and R.analyze("ab", (3, 3)) == [" ab", "ab "]
    keys, counts = R.row_counts("aaaa")
    assert [R.key_ngram(k) for k in keys] == [" a", " aa", "a ", "aa", "aa ", "aaa"] and counts.tolist() == [1, 1, 1, 3, 1, 2]


def test_key_is_exact_and_orders_like_the_strings():
    from snx.retrieval import keys_to_ngrams
    grams = [" ", " a", " a ", "a", "a ", "ab", "abc", "\U0010FFFF", "\U0010FFFF\U0010FFFF\U0010FFFF", "\U0001F600a",
             "한", "한 ", "한글", "z\U0010FFFF", "~", "\x7f\x7f"]
    keys = np.array([R.ngram_key(g) for g in grams], dtype=np.int64)    # U+10FFFF three times still fits int64
    assert (keys > 0).all()
    assert keys_to_ngrams(keys) == grams and [R.key_ngram(k) for k in keys.tolist()] == grams
    assert [grams[i] for i in np.argsort(keys)] == sorted(grams)         # a prefix sorts first: scikit-learn's order


def test_word_rows_and_ranges():
    from snx.retrieval import lds_row_capacity, word_rows
    from snx.retrieval.tfidf import check_ngram_range, slots_per_position
    ptr, cps = word_rows(["  Ab\t\tC \n", "", " \n", "İx"])
    assert ptr.tolist() == [0, 4, 4, 4, 7] and "".join(map(chr, cps)) == "ab c" + "İx".lower()
    assert lds_row_capacity((2, 3)) == 2046 and lds_row_capacity((1, 1)) == 2046 and lds_row_capacity((1, 3)) == 1022
    assert slots_per_position(1, 3) == 4 and slots_per_position(3, 3) == 1
    for bad in ((0, 2), (2, 1), (1, 4), (2,), "23", (1.0, 2), (True, 2)):
        with pytest.raises(ValueError):
            check_ngram_range(bad)
    with pytest.raises(ValueError):
        word_rows(["a", 3])


# ------------------------------------------------------------------------------------------------ the fit
def test_tie_rule_at_the_cut_keeps_the_lowest_keys():
    """Three n-grams with equal totals and max_features cutting through them: the lowest keys stay."""
    from snx.retrieval import select_features
    # the 1-grams of "b c d a a a": the blank 12, a 3, and b, c, d once each
    m = R.fit(["b c d a a a"], (1, 1), 4)
    assert [R.key_ngram(k) for k in m["keys"]] == [" ", "a", "b", "c"] and m["total"].tolist() == [12, 3, 1, 1]
    m = R.fit(["b c d a a a"], (1, 1), 3)
    assert [R.key_ngram(k) for k in m["keys"]] == [" ", "a", "b"]
    # the product's selection (torch, any device) over totals in ascending key order
    total = torch.tensor([12, 3, 1, 1, 1], dtype=torch.long)
    assert select_features(total, 4).tolist() == [0, 1, 2, 3] and select_features(total, 3).tolist() == [0, 1, 2]
    assert select_features(torch.tensor([1, 5, 1, 5, 1, 9]), 4).tolist() == [0, 1, 3, 5]
    assert select_features(total, None).tolist() == [0, 1, 2, 3, 4] and select_features(total, 5).tolist() == [0, 1, 2, 3, 4]
    assert select_features(total, 99).tolist() == [0, 1, 2, 3, 4]


def test_g17_features_and_idf_are_the_references(g17, model):
    assert g17["distinct_ngrams"] == model["distinct"] and g17["max_features"] < model["distinct"]
    assert [R.key_ngram(k) for k in model["keys"].tolist()] == g17["features"]
    assert model["idf"].dtype == np.float64 and np.array_equal(model["idf"], g17["arrays"]["idf"])     # bit-equal
    from snx.retrieval import tfidf_idf
    assert np.array_equal(tfidf_idf(model["doc_freq"], len(g17["corpus"])), g17["arrays"]["idf"])


def test_g17_corpus_weights_within_one_ulp(g17, model):
    a = g17["arrays"]
    rows = R.transform(g17["corpus"], model)
    assert len(rows) == a["corpus_indptr"].size - 1
    worst = 0
    for i, (fid, w) in enumerate(rows):
        lo, hi = a["corpus_indptr"][i], a["corpus_indptr"][i + 1]
        assert np.array_equal(fid, a["corpus_indices"][lo:hi])
        worst = max(worst, int(_ulps32(w, a["corpus_data"][lo:hi]).max()))
    assert worst <= 1


def test_g17_scores_of_the_restatement_within_the_bound(g17, model):
    from src.train.mining.tfidf import read_records
    a = g17["arrays"]
    recs = [read_records(f) for f in g17["input_files"]]
    q = [recs[s][i].get("query", "") for s, i in g17["need"]]
    q_rows = R.transform(q, model)
    assert [len(f) for f, _ in q_rows] == a["nnz_q"].tolist()
    F = model["keys"].size
    s32 = R.scores32(R.dense32(q_rows, F), R.dense32(R.transform(g17["corpus"], model), F))
    tol = np.array([R.mining_tolerance(n) for n in a["nnz_q"]])[:, None]
    assert (np.abs(s32.astype(np.float64) - a["scores"]) <= tol).all()


# ------------------------------------------------------------------------------------------------ the miner
def test_miner_on_the_stand_in_reproduces_the_reference(g17, tmp_path):
    from src.train.mining.tfidf import collect_shard_files, mine_tfidf_negatives
    src = tmp_path / "in"
    shutil.copytree(os.path.join(G17, "input"), src)
    files = collect_shard_files(str(src))
    assert [os.path.basename(f) for f in files] == g17["shards"]
    before = {f: open(f, "rb").read() for f in files}
    index = R.NumpyTfidfIndex((2, 3), g17["max_features"], True)
    out = mine_tfidf_negatives(files, index, output_dir=str(tmp_path / "out"), max_corpus=g17["max_corpus"],
                               top_k=g17["top_k"], batch_size=g17["batch_size"])
    assert out["corpus"] == len(g17["corpus"]) == index.num_docs and index.texts == g17["corpus"]
    seen = R.check_mining_output(g17, str(tmp_path / "out"), out["shards"])
    # the empty, the blank and the two unknown-n-gram queries, and one query whose n-grams all fell below the cut
    assert seen["zero"] == 5 and out["failed"] == 5 and seen["close"] == 0
    assert out["total"] == sum(s["total"] for s in g17["stats"])
    assert {f: open(f, "rb").read() for f in files} == before            # an output directory leaves the input alone
    assert sorted(os.listdir(tmp_path / "out")) == g17["shards"]         # no temporary file is left behind
    # a dry run writes nothing; in place rewrites the shards themselves, with the same records
    dry = mine_tfidf_negatives(files, R.NumpyTfidfIndex((2, 3), g17["max_features"]), output_dir=str(tmp_path / "dry"),
                               max_corpus=g17["max_corpus"], top_k=g17["top_k"], dry_run=True)
    assert not (tmp_path / "dry").exists() and dry["shards"] == out["shards"]
    mine_tfidf_negatives(files, R.NumpyTfidfIndex((2, 3), g17["max_features"]), max_corpus=g17["max_corpus"],
                         top_k=g17["top_k"], batch_size=1000)
    for n in g17["shards"]:
        assert open(src / n, "rb").read() == open(tmp_path / "out" / n, "rb").read()


def test_miner_edge_cases(tmp_path):
    from src.train.mining.tfidf import (build_positive_corpus, collect_shard_files, mine_tfidf_negatives, parse_shard_range,
                                        read_records)
    assert parse_shard_range("all", 3) == [0, 1, 2] and parse_shard_range("1-2", 5) == [1, 2] and parse_shard_range("4", 9) == [4]
    with pytest.raises(FileNotFoundError):
        collect_shard_files(str(tmp_path))
    recs = [{"query": "red apple", "positive": "a red apple pie"}, {"query": "green pear", "positive": "a green pear tart"},
            {"query": "red pear", "positive": "a red apple pie", "negative": "kept"}, {"query": "blue", "positive": ""},
            {"query": "zzz", "positive": "a green pear tart", "negative": None}]
    p = tmp_path / "train_shard_0.jsonl"
    with open(p, "w", encoding="utf-8") as f:
        f.write("\n".join(json.dumps(r) for r in recs[:2]) + "\n\nnot json\n" + "\n".join(json.dumps(r) for r in recs[2:]) + "\n")
    (tmp_path / "other.jsonl").write_text("{}\n")
    assert collect_shard_files(str(tmp_path), "0-3") == [str(p)]
    assert len(read_records(str(p))) == 5
    assert build_positive_corpus([str(p)], 10) == ["a red apple pie", "a green pear tart"]
    assert build_positive_corpus([str(p)], 1) == ["a red apple pie"]
    out = mine_tfidf_negatives([str(p)], R.NumpyTfidfIndex(), top_k=10)
    assert {k: out[k] for k in ("total", "already_had_negative", "added", "failed")} == \
        {"total": 5, "already_had_negative": 1, "added": 3, "failed": 1}
    got = read_records(str(p))
    assert got[0]["negative"] == "a green pear tart" and got[1]["negative"] == "a red apple pie"
    assert got[0]["difficulty"] == got[1]["difficulty"] == "hard" and got[2] == recs[2]
    assert got[3]["negative"] == "a red apple pie"            # "blue" shares "e " with "apple" and "pie" only
    assert "negative" not in got[4] or not got[4]["negative"]  # "zzz": no shared n-gram, never a zero-score negative
    # a corpus of one document that is the record's own positive: nothing admissible
    q = tmp_path / "one" / "train_shard_0.jsonl"
    q.parent.mkdir()
    q.write_text(json.dumps({"query": "red apple", "positive": "a red apple pie"}) + "\n")
    out = mine_tfidf_negatives([str(q)], R.NumpyTfidfIndex())
    assert out["failed"] == 1 and out["added"] == 0
    # no positives at all: the index is never built or searched
    q.write_text(json.dumps({"query": "red apple"}) + "\n")
    assert mine_tfidf_negatives([str(q)], R.NumpyTfidfIndex())["failed"] == 1


def test_cli_flags_equal_the_references(g17):
    from src.train.cli import mine_tfidf_negatives as cli
    ours = R.cli_flags_of(inspect.getsourcefile(cli))
    theirs = g17["cli_flags"]
    assert sorted(theirs) == ["--batch-size", "--corpus-chunk-size", "--data-dir", "--dry-run", "--max-corpus",
                              "--max-features", "--output-dir", "--shard-range", "--top-k"]
    assert {k: ours.get(k) for k in theirs} == theirs
    args = cli.parse_args([])
    assert (args.max_corpus, args.max_features, args.top_k, args.batch_size, args.shard_range, args.dry_run,
            args.output_dir, str(args.data_dir)) == (50000, 30000, 10, 1000, "all", False, None, "data/v29.0")


def test_header_python_and_kernel_agree_on_the_constants():
    from snx._lib import SIGNATURES
    from snx.retrieval import tfidf as T
    header = open(os.path.join(ROOT, "include", "snx.h"), encoding="utf-8").read()
    assert f"#define SNX_TFIDF_LDS_KEYS {T.LDS_KEYS}\n" in header
    for name in ("snx_tfidf_counts_workspace_bytes", "snx_tfidf_row_counts", "snx_tfidf_weights",
                 "snx_tfidf_compact_counts", "snx_tfidf_compact_rows"):
        assert name in SIGNATURES and f" {name}(" in header
