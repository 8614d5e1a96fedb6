"""CPU checks of the mid-training evaluator (src.train.eval): the reference call site's constructor, the corpus rules and
the metrics of ref:benchmark/metrics.py:52-99 (fixture tests/golden/g12_retrieval_metrics.json, written by
tools/make_golden_retrieval.py from the reference's own functions).  The GPU scorer is covered by test_gpu_retrieval.py."""
import inspect
import json
import logging
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G12 = os.path.join(ROOT, "tests", "golden", "g12_retrieval_metrics.json")


def _jsonl(path, recs):
    with open(path, "w") as f:
        for r in recs:
            f.write(json.dumps(r) + "\n")
    return str(path)


def test_evaluator_takes_the_reference_call_site_keywords(tmp_path):
    from src.train.data.collator import create_tokenizer
    from src.train.eval import MidTrainingEvaluator
    params = inspect.signature(MidTrainingEvaluator).parameters
    for name in ("tokenizer", "val_file", "max_queries", "max_docs", "device", "query_max_length", "doc_max_length"):
        assert name in params
    assert params["batch_size"].default == 64
    val = _jsonl(tmp_path / "val.jsonl", [{"query": "a b", "positive": "c d", "negative": "e f"}])
    # ref:src/train/cli/train_v33_ddp.py:633-641, verbatim keywords (construction needs no GPU)
    ev = MidTrainingEvaluator(tokenizer=create_tokenizer("hash:1000"), val_file=val, max_queries=200, max_docs=1000,
                              device="cpu", query_max_length=64, doc_max_length=256)
    assert ev.corpus.queries == ["a b"] and ev.corpus.docs == ["c d", "e f"] and ev.corpus.targets == [0]


def test_corpus_order_dedup_and_both_negative_schemas(tmp_path):
    from src.train.data import load_training_data
    from src.train.eval import build_eval_corpus
    recs = [{"query": "q0", "positive": "P0", "negative": "N0"},
            {"query": "q1", "positive": "P1", "negatives": ["N1a", "P0", "N1b"]},
            {"query": "q2", "positive": "P0", "negative": "N0"},                  # duplicate positive and negative
            {"query": "q3", "positive": "P3", "negatives": ["N3a", "N3b"]},
            {"query": "q4", "positive": "P4", "negative": "N4"}]
    ds = load_training_data([_jsonl(tmp_path / "v.jsonl", recs)])
    c = build_eval_corpus((ds[i] for i in range(len(ds))), max_queries=3, max_docs=100)
    assert c.queries == ["q0", "q1", "q2"]
    assert c.docs == ["P0", "P1", "N0", "N1a", "N1b", "P3", "N3a", "N3b", "P4", "N4"]
    assert c.targets == [0, 1, 0] and c.forced == 0


def test_corpus_limits_and_forced_positives():
    from src.train.eval import build_eval_corpus
    recs = [{"query": f"q{i}", "positive": f"P{i}", "negatives": [f"N{i}a", f"N{i}b"]} for i in range(6)]
    c = build_eval_corpus(recs, max_queries=2, max_docs=5)
    assert c.queries == ["q0", "q1"]
    assert c.docs == ["P0", "P1", "N0a", "N0b", "N1a"] and c.targets == [0, 1] and c.forced == 0
    # more queries than max_docs: every positive stays, the overshoot is counted, no negative gets in
    c = build_eval_corpus(recs, max_queries=4, max_docs=2)
    assert c.docs == ["P0", "P1", "P2", "P3"] and c.targets == [0, 1, 2, 3] and c.forced == 2
    c = build_eval_corpus(recs, max_queries=0, max_docs=3)
    assert c.queries == [] and c.docs == ["P0", "N0a", "N0b"]


def test_evaluator_logs_forced_positives(tmp_path, caplog):
    from src.train.data.collator import create_tokenizer
    from src.train.eval import MidTrainingEvaluator
    recs = [{"query": f"q{i}", "positive": f"P{i}", "negative": f"N{i}"} for i in range(4)]
    val = _jsonl(tmp_path / "val.jsonl", recs)
    with caplog.at_level(logging.INFO, logger="src.train.eval"):
        ev = MidTrainingEvaluator(create_tokenizer("hash:1000"), val, max_queries=4, max_docs=3, device="cpu")
    assert ev.corpus.forced == 1 and len(ev.corpus.docs) == 4
    assert any("kept past max_docs" in r.getMessage() for r in caplog.records)


def test_corpus_from_synthetic_pseudo_path():
    from src.train.data import load_training_data
    from src.train.data.collator import create_tokenizer
    from src.train.eval import MidTrainingEvaluator, build_eval_corpus
    ev = MidTrainingEvaluator(create_tokenizer("hash:1000"), "synthetic:40:3", max_queries=10, max_docs=25, device="cpu")
    ds = load_training_data(["synthetic:40:3"])
    again = build_eval_corpus((ds[i] for i in range(len(ds))), 10, 25)
    assert ev.corpus == again
    assert len(ev.corpus.queries) == 10 and len(ev.corpus.docs) == 25
    assert [ev.corpus.docs[t] for t in ev.corpus.targets] == [ds[i]["positive"] for i in range(10)]
    assert ev.corpus.docs[10:13] == ds[0]["negatives"]


def test_metrics_from_ranks_equal_reference_golden():
    from src.train.eval import metrics_from_ranks
    with open(G12) as f:
        g = json.load(f)
    assert len(g["cases"]) >= 8
    for case in g["cases"]:
        got = metrics_from_ranks(case["ranks"])
        assert got == case["metrics"], (case["name"], got, case["metrics"])


def test_sparse_index_validates_on_the_host():
    torch = pytest.importorskip("torch")
    from snx.retrieval import SparseIndex
    with pytest.raises(ValueError):
        SparseIndex(0, "cpu")
    idx = SparseIndex(16, "cpu")
    with pytest.raises(ValueError):                      # not a device tensor
        idx.add(torch.ones(2, 3), torch.zeros(2, 3, dtype=torch.int32), torch.ones(2, dtype=torch.int32))
    with pytest.raises(RuntimeError):
        idx.search(torch.ones(1, 1), torch.zeros(1, 1, dtype=torch.int32), torch.ones(1, dtype=torch.int32), 10)


def test_search_abi_rejects_bad_arguments_without_a_gpu():
    import ctypes as C
    from snx import fn
    one = C.c_void_p(16)
    srch = fn("snx_sparse_search")
    args = [one, one, one, 4, one, one, one, one, one, one, 100, 50, None, 10, 0, one, one, None, None, one, 1 << 20, None]
    bad_k = list(args); bad_k[13] = 1025
    assert srch(*bad_k) == -2
    bad_chunk = list(args); bad_chunk[14] = 32769
    assert srch(*bad_chunk) == -2
    no_out = list(args); no_out[15] = None
    assert srch(*no_out) == -3
    tgt_no_rank = list(args); tgt_no_rank[12] = one
    assert srch(*tgt_no_rank) == -3
    small_ws = list(args); small_ws[20] = 8
    assert srch(*small_ws) == -3
    assert fn("snx_sparse_search_workspace_bytes")(4, 100, 10, 0) >= 4 * 10 * 8
    assert fn("snx_sparse_index_workspace_bytes")(1000, 50000) >= 50000 * 8
    build = fn("snx_sparse_index_build")
    assert build(one, one, one, 10, 0, 5, one, one, one, one, 1 << 20, None) == -2
    assert build(one, one, one, 1000, 50000, 5, one, one, one, one, 8, None) == -3
