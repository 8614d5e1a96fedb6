"""SEISMIC on the GPU (csrc/seismic.hip via snx.retrieval.SeismicIndex), its evaluator keys and the CLI
src.train.cli.eval_seismic.  The contract (include/snx.h "SEISMIC") is deterministic, so the build structure, results,
ranks and counters must equal the numpy reference (tests/seismic_reference.py) BIT for BIT: with dyadic weights its
fp32 multiply-add is exact, with realistic fp32 weights it scores through SparseIndex.pair_scores (the ABI itself)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import seismic_reference as R
from tests.test_gpu_retrieval import _index, _rows, _tiny_model, _to_device, _val_file
from tests.test_seismic_host import (HAND_ALPHA, HAND_DOCS, HAND_DOCS_OUT, HAND_HF, HAND_K, HAND_NP, HAND_QUERIES,
                                     HAND_R, HAND_RANK, HAND_SCORES_OUT, HAND_STATS, HAND_STRUCT, HAND_TARGETS,
                                     HAND_TOP_N, HAND_TSCORE, HAND_V)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "opensearch-neural-pre-train_amd")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _bits(a):
    a = np.asarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same_structure(six, ref):
    got = six.structure()
    for key, want in ref.items():
        assert np.array_equal(_bits(got[key].numpy()), _bits(np.asarray(want).astype(got[key].numpy().dtype))), key


def _search_both(dev, six, ref, docs, queries, k, top_n, hf, targets, pair=R.dyadic_pairs, scores=None, **kw):
    qv, qi, qc = _to_device(queries, dev, np.random.default_rng(9))
    tg = torch.tensor(targets, dtype=torch.int32, device=dev)
    sc, dc, rk, ts, st = six.search(qv, qi, qc, k, top_n=top_n, heap_factor=hf, targets=tg, **kw)
    rs, rd, rr, rt, rst = R.search(ref, docs, queries, k, top_n, hf, targets, pair, scores)
    assert np.array_equal(dc.cpu().numpy(), rd), (k, top_n, hf)
    assert np.array_equal(_bits(sc.cpu().numpy()), _bits(rs)), (k, top_n, hf)
    assert np.array_equal(rk.cpu().numpy(), rr) and np.array_equal(_bits(ts.cpu().numpy()), _bits(rt))
    got = np.stack([st[x].cpu().numpy() for x in ("blocks_total", "blocks_scored", "postings_scored")], 1)
    assert np.array_equal(got, rst), (k, top_n, hf)
    return sc, dc, rk, ts, st


def test_hand_worked_example(dev):
    from snx.retrieval import SeismicIndex
    six = SeismicIndex(_index(R.rows32(HAND_DOCS), HAND_V, dev), HAND_NP, HAND_R, HAND_ALPHA)
    _same_structure(six, HAND_STRUCT)
    assert six.num_blocks == 7 and six.summary_nnz == 14 and six.build_seconds > 0
    qv, qi, qc = _to_device(R.rows32(HAND_QUERIES), dev)
    sc, dc, rk, ts, st = six.search(qv, qi, qc, HAND_K, top_n=HAND_TOP_N, heap_factor=HAND_HF,
                                    targets=torch.tensor(HAND_TARGETS, device=dev))
    assert dc.tolist() == HAND_DOCS_OUT and sc.tolist() == HAND_SCORES_OUT
    assert rk.tolist() == HAND_RANK and ts.tolist() == HAND_TSCORE
    assert torch.stack([st["blocks_total"], st["blocks_scored"], st["postings_scored"]], 1).tolist() == HAND_STATS


def _dyadic_corpus(seed, nd=120, V=16):
    rng = np.random.default_rng(seed)
    docs = _rows(rng, nd, V, 5, np.array([16, 32, 64]), empty_every=23)      # coarse levels: many weight / score ties
    for i in range(0, nd - 1, 17):
        docs[i + 1] = docs[i]                                              # duplicate docs
    queries = _rows(rng, 12, V, 6, np.array([16, 32, 64]), empty_every=11)
    targets = [int(rng.integers(0, nd)) for _ in queries]
    return docs, queries, targets


def test_dyadic_grid_bit_equal_to_the_reference(dev):
    from snx.retrieval import SeismicIndex
    docs, queries, targets = _dyadic_corpus(1)
    V = 16
    idx = _index(docs, V, dev)
    qgrid = [(k, t, h) for k in (1, 10, 1024) for t in (1, 3, 100) for h in (0.5, 1.0, 2.0, np.inf)]
    n = 0
    for n_postings in (1, 3, 17, 10 ** 6):
        for r in (0.01, 0.3, 1.0):
            for alpha in (0.05, 0.4, 1.0):
                six = SeismicIndex(idx, n_postings, r, alpha)
                ref = R.build(docs, V, n_postings, r, alpha)
                _same_structure(six, ref)
                scores = R.query_scores(ref, docs, queries)
                for k, t, h in qgrid[n % 6::6]:                          # every query setting over the grid
                    _search_both(dev, six, ref, docs, queries, k, t, h, targets, scores=scores)
                n += 1


def _fp32_corpus(rng, n, V, m):
    zipf = 1.0 / np.arange(1, V + 1)
    zipf /= zipf.sum()
    rows = []
    for _ in range(n):
        t = np.unique(rng.choice(V, size=m, p=zipf))
        rows.append((t, np.log1p(rng.uniform(0.05, 8.0, size=len(t))).astype(np.float32).astype(np.float64)))
    return rows


def test_fp32_weights_bit_equal_through_pair_scores(dev):
    from snx.retrieval import SeismicIndex
    rng = np.random.default_rng(2)
    V = 300
    docs, queries = _fp32_corpus(rng, 1500, V, 40), _fp32_corpus(rng, 16, V, 20)
    targets = [int(x) for x in rng.integers(0, len(docs), size=len(queries))]
    idx = _index(docs, V, dev)
    pair = R.gpu_pairs(dev)
    for n_postings, r, alpha in ((50, 0.1, 0.4), (17, 0.3, 0.05), (200, 0.05, 0.8)):
        six = SeismicIndex(idx, n_postings, r, alpha)
        ref = R.build(docs, V, n_postings, r, alpha, pair)
        _same_structure(six, ref)
        scores = R.query_scores(ref, docs, queries, pair)
        for k, t, h in ((10, 5, 1.0), (100, 10, 0.5), (10, 3, 2.0)):
            sc, dc, rk, ts, _ = _search_both(dev, six, ref, docs, queries, k, t, h, targets, pair, scores)
            # every returned score and the target score are the exact index's pair scores, bit for bit
            qv, qi, qc = _to_device(queries, dev)
            live = dc >= 0
            qrow = torch.arange(len(queries), device=dev)[:, None].expand_as(dc)
            ps = idx.pair_scores(qv, qi, qc, torch.stack([qrow[live], dc[live].long()], 1))
            assert torch.equal(ps.view(torch.int32), sc[live].view(torch.int32))
            pt = idx.pair_scores(qv, qi, qc, torch.stack([torch.arange(len(queries), device=dev),
                                                          torch.tensor(targets, device=dev)], 1))
            assert torch.equal(pt.view(torch.int32), ts.view(torch.int32))


def test_degenerate_setting_is_exact_search_at_100k_docs(dev):
    from snx.retrieval import SeismicIndex
    rng = np.random.default_rng(3)
    V = 64
    docs = _rows(rng, 100_003, V, 12, np.arange(1, 5) * 16, common=3)
    queries = _rows(rng, 32, V, 10, np.arange(1, 5) * 16)
    idx = _index(docs, V, dev)
    qv, qi, qc = _to_device(queries, dev)
    tg = torch.tensor(rng.integers(0, len(docs), size=len(queries)), device=dev)
    six = SeismicIndex(idx, 200_000, 0.001, 0.3)
    for k in (10, 1024):
        es, ed, er, et = idx.search(qv, qi, qc, k, targets=tg)
        ss, sd, sr, st, stats = six.search(qv, qi, qc, k, top_n=1024, heap_factor=float("inf"), targets=tg)
        assert torch.equal(sd, ed) and torch.equal(ss.view(torch.int32), es.view(torch.int32))
        assert torch.equal(sr, torch.where(er <= k, er, torch.zeros_like(er)))
        assert torch.equal(st.view(torch.int32), et.view(torch.int32))
        assert torch.equal(stats["blocks_scored"], stats["blocks_total"])


def test_build_and_search_are_byte_identical_across_runs_and_slices(dev):
    from snx.retrieval import SeismicIndex
    rng = np.random.default_rng(4)
    V = 500
    docs, queries = _fp32_corpus(rng, 20000, V, 60), _fp32_corpus(rng, 40, V, 30)
    idx = _index(docs, V, dev)
    a, b = SeismicIndex(idx, 300, 0.1, 0.4), SeismicIndex(idx, 300, 0.1, 0.4)
    sa, sb = a.structure(), b.structure()
    for key in sa:
        assert torch.equal(sa[key].view(torch.int32) if sa[key].dtype == torch.float32 else sa[key],
                           sb[key].view(torch.int32) if sb[key].dtype == torch.float32 else sb[key]), key
    qv, qi, qc = _to_device(queries, dev)
    tg = torch.tensor(rng.integers(0, len(docs), size=len(queries)), device=dev)
    runs = [s.search(qv, qi, qc, 50, top_n=10, heap_factor=1.0, targets=tg, query_slice=q)
            for s, q in ((a, 0), (a, 0), (b, 1), (a, 7))]
    for r in runs[1:]:
        assert torch.equal(r[0].view(torch.int32), runs[0][0].view(torch.int32)) and torch.equal(r[1], runs[0][1])
        assert torch.equal(r[2], runs[0][2]) and torch.equal(r[3].view(torch.int32), runs[0][3].view(torch.int32))
        assert all(torch.equal(r[4][x], runs[0][4][x]) for x in r[4])


def test_edge_cases_and_the_query_cap(dev):
    from snx.retrieval import SEISMIC_Q_MAX, SeismicIndex
    rng = np.random.default_rng(5)
    V = 1200                                                              # terms 1100.. have no postings
    docs = [(np.sort(rng.choice(1100, size=int(rng.integers(1, 30)), replace=False)), None) for _ in range(300)]
    docs = [(t, rng.choice(np.array([16, 32, 64]) / 64.0, len(t))) for t, _ in docs]
    docs[5] = docs[77] = (np.zeros(0, np.int64), np.zeros(0))            # docs with no terms
    queries = [(np.zeros(0, np.int64), np.zeros(0)),                      # empty query row
               (np.array([1150]), np.array([1.0])),                       # a term with no postings
               (np.sort(rng.choice(V, size=SEISMIC_Q_MAX, replace=False)),  # at the cap, every weight tied
                np.full(SEISMIC_Q_MAX, 0.25))]
    targets = [5, 3, 9]
    idx = _index(docs, V, dev)
    six = SeismicIndex(idx, 40, 0.3, 0.4)
    ref = R.build(docs, V, 40, 0.3, 0.4)
    _same_structure(six, ref)
    sc, dc, rk, ts, st = _search_both(dev, six, ref, docs, queries, 1024, 2000, 1.0, targets)
    assert (dc[0] == -1).all() and (dc[1] == -1).all() and int((dc[2] >= 0).sum()) < 1024   # fewer docs than k
    assert int(st["blocks_total"][1]) == 0 and float(ts[0]) == 0.0
    too_long = [(np.arange(SEISMIC_Q_MAX + 1), np.full(SEISMIC_Q_MAX + 1, 0.5))]
    with pytest.raises(ValueError):
        six.search(*_to_device(too_long, dev), 10)
    q = _to_device(queries[:1], dev)
    for kw in ({"k": 0}, {"k": 1025}, {"k": 5, "top_n": 0}, {"k": 5, "heap_factor": 0.0},
               {"k": 5, "heap_factor": float("nan")}):
        with pytest.raises(ValueError):
            six.search(*q, **kw)
    for bad in ({"n_postings": 0}, {"cluster_ratio": 0.0}, {"cluster_ratio": 1.5}, {"summary_prune_ratio": 0.0},
                {"n_postings": 2.5}):
        with pytest.raises(ValueError):
            SeismicIndex(idx, **bad)


# ------------------------------------------------------------------------------------------------ evaluator and CLI
def test_evaluator_seismic_keys(dev, tmp_path):
    from src.train.data.collator import create_tokenizer
    from src.train.eval import MidTrainingEvaluator
    tok = create_tokenizer("hash:1000")
    model = _tiny_model(dev, tmp_path)
    val = _val_file(tmp_path)
    kw = dict(tokenizer=tok, val_file=val, max_queries=30, max_docs=90, device=str(dev), query_max_length=16,
              doc_max_length=32, batch_size=16)
    plain = MidTrainingEvaluator(**kw).evaluate(model)
    assert set(plain) == {"recall@1", "recall@5", "recall@10", "mrr@10", "ndcg@10", "num_queries", "num_docs",
                          "avg_nnz_q", "avg_nnz_d"}
    degenerate = MidTrainingEvaluator(**kw, seismic={"n_postings": 10 ** 6, "top_n": 1024,
                                                     "heap_factor": float("inf")}).evaluate(model)
    for key, v in plain.items():
        assert degenerate[key] == v, key
    for key in ("recall@1", "recall@5", "recall@10", "mrr@10", "ndcg@10"):
        assert degenerate[f"seismic_{key}"] == plain[key], key
    assert degenerate["seismic_overlap@5"] == 1.0 and degenerate["seismic_postings_frac"] == 1.0
    default = MidTrainingEvaluator(**kw, seismic={}).evaluate(model)
    extra = {k: v for k, v in default.items() if k.startswith("seismic_")}
    assert len(extra) == 7 and all(0.0 <= v <= 1.0 for v in extra.values()), extra


def test_cli_reference_sweep_end_to_end(dev, tmp_path):
    from src.model.splade_modern import SPLADEModernBERT
    mdir = tmp_path / "model"
    mdir.mkdir()
    (mdir / "config.json").write_text(json.dumps(dict(
        vocab_size=1000, hidden_size=256, intermediate_size=384, num_hidden_layers=2, num_attention_heads=4,
        local_attention=16, pad_token_id=999)))
    torch.manual_seed(5)
    (tmp_path / "ckpt").mkdir()
    torch.save(SPLADEModernBERT(model_name=str(mdir)).state_dict(), tmp_path / "ckpt" / "model.pt")
    val = _val_file(tmp_path, 80)
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "src.train.cli.eval_seismic", "--checkpoint", str(tmp_path / "ckpt"),
           "--model-name", str(mdir), "--tokenizer", "hash:1000", "--val-file", val, "--max-queries", "40",
           "--max-docs", "120", "--query-max-length", "16", "--doc-max-length", "32", "--batch-size", "16",
           "--reference-sweep"]
    outs = []
    for _ in range(2):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=str(tmp_path))
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
        outs.append([json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")])
    lines = outs[0]
    assert len(lines) == 21
    fields = {"n_postings", "cluster_ratio", "summary_prune_ratio", "top_n", "heap_factor", "recall@10",
              "seismic_recall@10", "seismic_mrr@10", "overlap@5", "blocks_scored", "postings_scored", "build_s",
              "search_s"}
    assert all(fields <= set(line) for line in lines)
    assert [line["n_postings"] for line in lines[:6]] == [10, 50, 100, 300, 500, 1000]
    assert [line["heap_factor"] for line in lines[14:]] == [1.0, 0.5, 1.0, 2.0, 1.0, 1.0, 1.0]

    def strip(ls):
        return [{k: v for k, v in line.items() if k not in ("build_s", "search_s")} for line in ls]
    assert strip(outs[0]) == strip(outs[1])
