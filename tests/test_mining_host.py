"""CPU checks of the hard-negative miner (src.train.mining, CLI src.train.cli.mine_negatives): corpus rules, band /
sampling / padding rules on hand-made bands, teacher fields, metadata, val files, CLI parsing, and the C ABI's argument
checks of snx_sparse_search_band / snx_sparse_pair_scores.  The GPU side is covered by test_gpu_mining.py."""
import json
import os

import numpy as np
import pytest


def _jsonl(path, recs):
    with open(path, "w") as f:
        for r in recs:
            f.write(json.dumps(r) + "\n")
    return str(path)


RECS_A = [{"query": "q0", "positive": "P0", "negative": "N0"},
          {"query": "q1", "positive": "P1", "negatives": ["N1a", "P0", "N1b"]},
          {"query": "q0", "positive": "P2", "negative": "N1a", "pair_type": "qd", "source": "s"}]
RECS_B = [{"query": "q2", "positive": "P3", "negatives": ["N0", "N3"], "negative": "N4"},
          {"query": "q1", "positive": "P1", "negatives": ["N5"]}]


def _corpus(tmp_path):
    from src.train.mining import build_corpus
    b = _jsonl(tmp_path / "b.jsonl", RECS_B)
    a = _jsonl(tmp_path / "a.jsonl", RECS_A)
    return build_corpus([b, a])                               # sorted: a.jsonl first


def test_corpus_order_dedup_over_all_three_negative_schemas(tmp_path):
    c = _corpus(tmp_path)
    assert [os.path.basename(f) for f in c.files] == ["a.jsonl", "b.jsonl"]
    assert c.docs == ["P0", "N0", "P1", "N1a", "N1b", "P2", "P3", "N4", "N3", "N5"]
    assert c.queries == ["q0", "q1", "q2"]
    assert c.rec_file == [0, 0, 0, 1, 1]
    assert c.rec_negs == [[1], [3, 0, 4], [3], [7, 1, 8], [9]]


def test_several_positives_group_under_one_query(tmp_path):
    c = _corpus(tmp_path)
    assert c.positives == [[0, 5], [2], [6]]
    assert c.rec_query == [0, 1, 0, 2, 1] and c.rec_pos == [0, 2, 5, 6, 2]


def test_length_batches_depend_on_the_corpus_only():
    from src.train.mining import length_batches
    assert length_batches([3, 1, 3, 2, 1], 2) == [[1, 4], [3, 0], [2]]
    assert length_batches([], 4) == []


def _assign(band, k=3, sample="first", seed=0, qid=0, orig=(), teacher="none", rec=None, positives=(0,)):
    from src.train.mining import assign_record
    docs = [f"D{i}" for i in range(20)]
    rec = rec or {"query": "q", "positive": "D0", "negatives": ["D7"], "teacher_pos_score": 0.7,
                  "teacher_neg_scores": [0.1]}
    return assign_record(rec, list(positives), list(orig), band, k, sample, seed, qid, docs, 2.5,
                         lambda d: 0.25 * d, teacher)


def test_first_takes_the_band_in_rank_order_and_pads_with_the_last():
    band = [(4, 3.0), (9, 2.0), (2, 1.5), (5, 1.0)]
    out, st = _assign(band)
    assert st == "full" and out["negatives"] == ["D4", "D9", "D2"] and out["miner_neg_scores"] == [3.0, 2.0, 1.5]
    assert out["miner_pos_score"] == 2.5
    out, st = _assign(band[:2])
    assert st == "padded" and out["negatives"] == ["D4", "D9", "D9"] and out["miner_neg_scores"] == [3.0, 2.0, 2.0]


def test_empty_band_falls_back_to_original_negatives_then_leaves_the_record():
    out, st = _assign([], orig=[0, 6, 6, 8], positives=(0,))
    assert st == "fallback" and out["negatives"] == ["D6", "D8", "D8"] and out["miner_neg_scores"] == [1.5, 2.0, 2.0]
    rec = {"query": "q", "positive": "D0", "negative": "D0", "teacher_pos_score": 0.5}
    out, st = _assign([], orig=[0], rec=rec)
    assert st == "unchanged" and out is rec


def test_random_sampling_is_keyed_on_seed_and_query():
    from src.train.mining import sample_band
    a = sample_band(40, 7, "random", 3, 11)
    assert a == sorted(a) and len(set(a)) == 7 and max(a) < 40
    assert sample_band(40, 7, "random", 3, 11) == a            # the same whatever slice of queries a rank holds
    assert sample_band(40, 7, "random", 4, 11) != a or sample_band(40, 7, "random", 3, 12) != a
    assert sample_band(5, 7, "random", 3, 11) == [0, 1, 2, 3, 4]
    band = [(i, 10.0 - i) for i in range(10)]
    out, _ = _assign(band, k=4, sample="random", seed=3, qid=11)
    assert out["negatives"] == [f"D{i}" for i in sample_band(10, 4, "random", 3, 11)]


def test_teacher_fields_dropped_by_default_and_self_written_on_request():
    band = [(4, 3.0), (9, 2.0), (2, 1.5)]
    out, _ = _assign(band)
    assert not any(k.startswith("teacher") for k in out)
    out, _ = _assign(band, teacher="self")
    assert out["teacher_pos_score"] == 2.5 and out["teacher_neg_scores"] == [3.0, 2.0, 1.5]


def test_metadata_kept_and_scores_written_as_fp32():
    from src.train.mining import f32
    rec = {"query": "q", "positive": "D0", "negative": "D1", "pair_type": "qd", "difficulty": "hard",
           "source": "s", "other": 1}
    out, _ = _assign([(3, 0.1)], k=1, rec=rec)
    assert out["pair_type"] == "qd" and out["difficulty"] == "hard" and out["source"] == "s" and "other" not in out
    assert list(out)[:5] == ["query", "positive", "negatives", "miner_pos_score", "miner_neg_scores"]
    assert np.float32(f32(np.float32(1 / 3))) == np.float32(1 / 3) and f32(0.1) == 0.1


def test_val_files_are_copied(tmp_path):
    from src.train.mining import copy_val_files
    v = tmp_path / "in"
    v.mkdir()
    _jsonl(v / "val.jsonl", RECS_A)
    out = tmp_path / "out"
    out.mkdir()
    got = copy_val_files([str(v / "val*.jsonl"), str(v / "missing.jsonl")], str(out))
    assert [os.path.basename(p) for p in got] == ["val.jsonl"]
    assert (out / "val.jsonl").read_bytes() == (v / "val.jsonl").read_bytes()


def test_cli_parsing_follows_the_reference_flags():
    from src.train.cli.mine_negatives import parse_args
    a = parse_args([])
    assert (a.k, a.rank_start, a.rank_end, a.query_top_k, a.sample, a.teacher_scores, a.max_score_ratio,
            a.chunk_docs) == (7, 10, 50, 64, "first", "none", None, 0)
    a = parse_args(["--input-pattern", "x/*.jsonl", "--output-dir", "o", "--k", "5", "--rank-start", "0",
                    "--rank-end", "30", "--checkpoint", "ck", "--tokenizer", "hash:50000", "--max-score-ratio", "0.95",
                    "--sample", "random", "--seed", "7", "--teacher-scores", "self", "--chunk-docs", "4096",
                    "--query-max-length", "32", "--doc-max-length", "128", "--batch-size", "8"])
    assert (a.input_pattern, a.k, a.rank_end, a.max_score_ratio, a.sample, a.seed, a.teacher_scores) == \
        ("x/*.jsonl", 5, 30, 0.95, "random", 7, "self")
    for bad in (["--rank-start", "50"], ["--rank-end", "2000"], ["--k", "0"], ["--sample", "top"],
                ["--max-score-ratio", "0"]):
        with pytest.raises(SystemExit):
            parse_args(bad)


def test_exclusion_rows_are_sorted_deduplicated_and_validated():
    torch = pytest.importorskip("torch")
    from snx.retrieval import exclusion_csr
    ptr, docs = exclusion_csr([[5, 1, 5], [], [9, 0]], 3, 10, "cpu")
    assert ptr.tolist() == [0, 2, 2, 4] and docs.tolist() == [1, 5, 0, 9] and docs.dtype == torch.int32
    ptr, docs = exclusion_csr((torch.tensor([0, 3, 3]), torch.tensor([7, 2, 7])), 2, 10, "cpu")   # unsorted row
    assert ptr.tolist() == [0, 2, 2] and docs.tolist() == [2, 7]
    with pytest.raises(ValueError):
        exclusion_csr([[1], [10]], 2, 10, "cpu")                  # out of range
    with pytest.raises(ValueError):
        exclusion_csr([[1]], 2, 10, "cpu")                        # one row per query
    with pytest.raises(ValueError):
        exclusion_csr((torch.tensor([0, 2, 1]), torch.tensor([1, 2])), 2, 10, "cpu")   # ptr decreases


def test_band_abi_rejects_bad_arguments_without_a_gpu():
    from snx import fn
    import ctypes as C
    one = C.c_void_p(16)
    band = fn("snx_sparse_search_band")
    # q_ptr, q_term, q_w, nq, term_ptr, post_doc, post_w, nd, V, ex_ptr, ex_doc, ceiling, lo, hi, chunk, out x3, ws, bytes
    args = [one, one, one, 4, one, one, one, 100, 50, one, one, one, 10, 50, 0, one, one, one, one, 1 << 30, None]
    for i, v, rc in ((12, 50, -2), (12, 60, -2), (12, -1, -2), (13, 1025, -2), (14, 32769, -2), (15, None, -3),
                     (16, None, -3), (17, None, -3), (10, None, -3), (19, 8, -3), (18, None, -3)):
        bad = list(args)
        bad[i] = v
        assert band(*bad) == rc, (i, v)
    assert fn("snx_sparse_search_band_workspace_bytes")(4, 100, 50, 0) >= 4 * 50 * 8
    assert fn("snx_sparse_search_band_workspace_bytes")(4, 100, 0, 0) == 0
    pair = fn("snx_sparse_pair_scores")
    assert pair(one, one, one, 4, one, one, one, 100, one, one, -1, one, None) == -2
    assert pair(one, one, one, 4, one, one, one, 100, None, one, 5, one, None) == -3
    assert pair(one, one, one, 4, one, one, one, 100, one, one, 5, None, None) == -3
    assert pair(None, one, one, 4, one, one, one, 100, one, one, 5, one, None) == -3
    assert pair(one, one, one, 4, one, one, one, 100, None, None, 0, None, None) == 0


def test_sparse_index_band_entry_points_validate_on_the_host():
    torch = pytest.importorskip("torch")
    from snx.retrieval import SparseIndex
    idx = SparseIndex(16, "cpu")
    q = (torch.ones(1, 1), torch.zeros(1, 1, dtype=torch.int32), torch.ones(1, dtype=torch.int32))
    with pytest.raises(ValueError):
        idx.search_band(*q, 5, 5)                                 # lo >= hi
    with pytest.raises(ValueError):
        idx.search_band(*q, 0, 1025)
    with pytest.raises(RuntimeError):
        idx.search_band(*q, 0, 10)                                # not built
    with pytest.raises(RuntimeError):
        idx.pair_scores(*q, torch.zeros(1, 2, dtype=torch.long))
