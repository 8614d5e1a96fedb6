"""Pruning and two-phase search on the GPU (csrc/two_phase.hip via snx.retrieval.prune_rows / SparseIndex.pruned /
rescore / search_two_phase), the evaluator's two_phase_* keys and the CLI src.train.cli.eval_pruning.  The contract
(include/snx.h "pruning and two-phase search") is deterministic, so keep flags, results, ranks and counters must equal
the numpy reference (tests/two_phase_reference.py) BIT for BIT on dyadic weights; with arbitrary fp32 weights every
returned score must be SparseIndex.pair_scores' (the ABI itself) and the output the top k of the phase-1 window."""
import json

import numpy as np
import pytest
import torch

from tests import two_phase_reference as R
from tests.test_gpu_retrieval import _index, _rows, _tiny_model, _to_device, _val_file
from tests.test_gpu_seismic import _fp32_corpus
from tests.test_two_phase_host import (HAND_DOCS, HAND_DOCS_OUT, HAND_K, HAND_MAXW, HAND_PRUNE, HAND_QUERIES, HAND_RANK,
                                       HAND_RATE, HAND_ROW, HAND_SCORES_OUT, HAND_STATS, HAND_TARGETS, HAND_TSCORE,
                                       HAND_TYPE, HAND_V, HAND_VALUE)

pytestmark = pytest.mark.gpu

LEVELS = np.array([16, 32, 64])                                           # coarse: many weight and score ties
STAT_KEYS = ("postings_high", "postings_all", "window_filled")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _bits(a):
    a = np.asarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _csr(rows, dev):
    rows = R.rows32(rows)
    cnt = torch.tensor([len(t) for t, _ in rows], dtype=torch.long, device=dev)
    terms = np.concatenate([t for t, _ in rows] + [np.zeros(0, np.int64)]).astype(np.int32)
    w = np.concatenate([w for _, w in rows] + [np.zeros(0, np.float32)]).astype(np.float32)
    return cnt, torch.from_numpy(terms).to(dev), torch.from_numpy(w).to(dev)


def _same_rows(got, want, what):
    cnt, terms, w = (x.cpu().numpy() for x in got)
    assert cnt.tolist() == [len(t) for t, _ in want], what
    assert np.array_equal(terms, np.concatenate([t for t, _ in want] + [np.zeros(0, np.int64)])), what
    assert np.array_equal(_bits(w), _bits(np.concatenate([x for _, x in want] + [np.zeros(0, np.float32)]))), what


def _same_search(got, want, what):
    sc, dc, rk, ts, st = got
    rs, rd, rr, rt, rst = want
    assert np.array_equal(dc.cpu().numpy(), rd), what
    assert np.array_equal(_bits(sc.cpu().numpy()), _bits(rs)), what
    assert np.array_equal(rk.cpu().numpy(), rr) and np.array_equal(_bits(ts.cpu().numpy()), _bits(rt)), what
    assert np.array_equal(np.stack([st[x].cpu().numpy() for x in STAT_KEYS], 1), rst), what
    assert all(st[x].dtype == torch.long for x in STAT_KEYS)


def test_hand_worked_example(dev):
    from snx.retrieval import prune_rows
    for ptype, value, want in HAND_PRUNE:
        kept, rest = prune_rows(*_csr([HAND_ROW, ([], []), ([3], [0.25])], dev), ptype, value)
        assert kept[1][:int(kept[0][0])].tolist() == [t for t, m in zip(HAND_ROW[0], want) if m], (ptype, value)
        assert rest[1][:int(rest[0][0])].tolist() == [t for t, m in zip(HAND_ROW[0], want) if not m], (ptype, value)
        assert int(kept[0][1]) == 0 and int(rest[0][1]) == 0
    idx = _index(R.rows32(HAND_DOCS), HAND_V, dev)
    qv, qi, qc = _to_device(R.rows32(HAND_QUERIES), dev)
    sc, dc, rk, ts, st = idx.search_two_phase(qv, qi, qc, HAND_K, HAND_TYPE, HAND_VALUE, HAND_RATE, HAND_MAXW,
                                              targets=torch.tensor(HAND_TARGETS, device=dev))
    assert dc.tolist() == HAND_DOCS_OUT and sc.tolist() == HAND_SCORES_OUT
    assert rk.tolist() == HAND_RANK and ts.tolist() == HAND_TSCORE
    assert torch.stack([st[x] for x in STAT_KEYS], 1).tolist() == HAND_STATS


PRUNE_GRID = [("max_ratio", v) for v in (0.0, 0.4, 0.5, 1.0)] + [("abs_value", v) for v in (0.25, 0.5, 0.6, 2.0)] + \
             [("top_k", v) for v in (1, 3, 40, 49999, 10 ** 6)] + [("alpha_mass", v) for v in (0.01, 0.4, 0.8, 1.0)]


def test_prune_rows_equals_the_reference_on_short_and_whole_vocabulary_rows(dev):
    from snx.retrieval import prune_rows
    rng = np.random.default_rng(1)
    V = 50_000
    short = _rows(rng, 300, 64, 40, LEVELS, empty_every=13)
    short[1] = short[2] = (np.array([7]), np.array([0.5]))                 # single-entry rows
    short[3] = (np.arange(40), np.full(40, 0.25))                          # every weight tied
    whole = (np.arange(V), rng.choice(LEVELS, V) / 64.0)                   # a random-init model's row: the workspace path
    mid = (np.sort(rng.choice(V, 5000, replace=False)), rng.choice(LEVELS, 5000) / 64.0)
    at_lds = (np.arange(4096), rng.choice(LEVELS, 4096) / 64.0)            # the longest row that sorts in LDS
    for rows in (short, short[:40] + [whole] + short[40:80] + [mid, at_lds, ([], [])]):
        csr = _csr(rows, dev)
        before = [x.clone() for x in csr]
        for ptype, value in PRUNE_GRID:
            kept, rest = prune_rows(*csr, ptype, value)
            want_kept, want_rest = R.prune(rows, ptype, value)
            _same_rows(kept, want_kept, (ptype, value, "kept"))
            _same_rows(rest, want_rest, (ptype, value, "rest"))
        assert all(torch.equal(a, b) for a, b in zip(csr, before))


def _dyadic_corpus(seed, nd, V, nq, q_nnz=10):
    rng = np.random.default_rng(seed)
    docs = _rows(rng, nd, V, 12, LEVELS, empty_every=97)
    for i in range(0, nd - 1, 41):
        docs[i + 1] = docs[i]                                              # duplicate docs: score ties
    queries = _rows(rng, nq, V, q_nnz, np.array([8, 16, 24, 32, 64]), empty_every=11)
    targets = [int(x) for x in rng.integers(0, nd, size=nq)]
    return rng, docs, queries, targets


def test_rescore_equals_the_reference(dev):
    V = 1500
    rng, docs, queries, targets = _dyadic_corpus(2, 600, V, 14)
    queries[3] = (np.sort(rng.choice(V, 1200, replace=False)), np.full(1200, 0.25))   # longer than the LDS staging
    queries[4] = (np.arange(1024), np.full(1024, 0.5))                     # exactly at it
    idx = _index(docs, V, dev)
    S = R.scores(queries, docs, V)
    qv, qi, qc = _to_device(queries, dev, np.random.default_rng(9))
    tg = torch.tensor(targets, dtype=torch.int32, device=dev)
    for W, k in ((1, 1), (37, 10), (64, 64), (200, 7), (1024, 1024), (1024, 10)):
        cand = rng.integers(-1, len(docs), size=(len(queries), W))
        cand[:, W // 2:] = np.where(rng.random((len(queries), W - W // 2)) < 0.3, -1, cand[:, W // 2:])   # -1 slots
        if W > 4:
            cand[:, 3] = cand[:, 0]                                        # a doc given twice
            cand[5] = -1                                                   # an empty window
        got = idx.rescore(qv, qi, qc, torch.from_numpy(cand.astype(np.int32)).to(dev), k, targets=tg)
        want = R.rescore(S, cand, k, targets)
        assert np.array_equal(got[1].cpu().numpy(), want[1]), (W, k)
        assert np.array_equal(_bits(got[0].cpu().numpy()), _bits(want[0])), (W, k)
        assert np.array_equal(got[2].cpu().numpy(), want[2]) and \
            np.array_equal(_bits(got[3].cpu().numpy()), _bits(want[3])), (W, k)
        assert (S[np.arange(len(queries))[:, None], np.maximum(cand, 0)] == 0).any()   # candidates that score 0 were given
    sc, dc, rk, ts = idx.rescore(qv, qi, qc, torch.full((len(queries), 5), -1, dtype=torch.int32, device=dev), 2)
    assert rk is None and ts is None and (dc == -1).all() and (sc == 0).all()
    for cand, k in ((torch.zeros((len(queries), 0), dtype=torch.int32, device=dev), 1),
                    (torch.zeros((len(queries), 1025), dtype=torch.int32, device=dev), 10),
                    (torch.zeros((len(queries), 8), dtype=torch.int32, device=dev), 9),
                    (torch.zeros((len(queries), 8), dtype=torch.int64, device=dev), 2),
                    (torch.zeros((3, 8), dtype=torch.int32, device=dev), 2)):
        with pytest.raises(ValueError):
            idx.rescore(qv, qi, qc, cand, k)


TWO_PHASE_GRID = [("max_ratio", 0.4, 5.0), ("top_k", 3, 2.0), ("alpha_mass", 0.6, 10.0), ("abs_value", 0.5, 1.0)]


def test_search_two_phase_equals_the_reference(dev):
    V = 200
    _, docs, queries, targets = _dyadic_corpus(3, 3000, V, 24)
    idx = _index(docs, V, dev)
    qv, qi, qc = _to_device(queries, dev, np.random.default_rng(9))
    tg = torch.tensor(targets, dtype=torch.int32, device=dev)
    for ptype, value, rate in TWO_PHASE_GRID:                              # the reference setting first
        got = idx.search_two_phase(qv, qi, qc, 10, ptype, value, rate, 10000, targets=tg)
        _same_search(got, R.two_phase(docs, queries, V, 10, ptype, value, rate, 10000, targets), (ptype, value, rate))
    got = idx.search_two_phase(qv, qi, qc, 10, "max_ratio", 0.4, 50.0, 64, targets=tg)       # the window cap binds
    _same_search(got, R.two_phase(docs, queries, V, 10, "max_ratio", 0.4, 50.0, 64, targets), "max_window_size")
    defaults = idx.search_two_phase(qv, qi, qc, 10, targets=tg)            # the defaults are the reference setting
    _same_search(defaults, R.two_phase(docs, queries, V, 10, targets=targets), "defaults")
    with pytest.raises(ValueError):
        idx.search_two_phase(qv, qi, qc, 10, expansion_rate=200.0)


def _rows_of(csr):
    cnt, terms, w = (x.cpu().numpy() for x in csr)
    ends = np.cumsum(cnt)
    return [(terms[e - c:e].astype(np.int64), w[e - c:e].astype(np.float64)) for c, e in zip(cnt, ends)]


def test_fp32_weights_scores_are_pair_scores_and_the_output_is_the_top_of_the_window(dev):
    from snx.retrieval import pack_rows, prune_rows, two_phase_window
    rng = np.random.default_rng(4)
    V, k = 300, 10
    docs, queries = _fp32_corpus(rng, 4000, V, 40), _fp32_corpus(rng, 16, V, 20)
    idx = _index(docs, V, dev)
    qv, qi, qc = _to_device(queries, dev)
    tg = torch.tensor(rng.integers(0, len(docs), size=len(queries)), dtype=torch.int32, device=dev)
    qrow = torch.arange(len(queries), device=dev)
    for ptype, value, rate in TWO_PHASE_GRID:
        sc, dc, rk, ts, st = idx.search_two_phase(qv, qi, qc, k, ptype, value, rate, 10000, targets=tg)
        live = dc >= 0
        ps = idx.pair_scores(qv, qi, qc, torch.stack([qrow[:, None].expand_as(dc)[live], dc[live].long()], 1))
        assert torch.equal(ps.view(torch.int32), sc[live].view(torch.int32)) and (sc[~live] == 0).all()
        pt = idx.pair_scores(qv, qi, qc, torch.stack([qrow, tg.long()], 1))
        assert torch.equal(pt.view(torch.int32), ts.view(torch.int32))
        # the phase-1 window, from the public pieces: exact search over the pruned query rows at k = W
        W = two_phase_window(k, rate, 10000)
        high, _ = prune_rows(*pack_rows(qv, qi, qc, V), ptype, value)
        _, C, _, _ = idx.search(*_to_device(_rows_of(high), dev), W)
        assert torch.equal(st["window_filled"], (C >= 0).sum(1))
        cs = idx.pair_scores(qv, qi, qc, torch.stack([qrow[:, None].expand_as(C).reshape(-1),
                                                      C.clamp(min=0).long().reshape(-1)], 1)).view(len(queries), W)
        C, cs = C.cpu().numpy(), cs.cpu().numpy()
        for q in range(len(queries)):
            ok = (C[q] >= 0) & (cs[q] > 0)
            d, s = C[q][ok], cs[q][ok]
            o = np.lexsort((d, -s.astype(np.float64)))[:k]
            assert dc[q, :len(o)].tolist() == d[o].tolist() and (dc[q, len(o):] == -1).all(), (ptype, q)
            assert int(rk[q]) == next((r + 1 for r, x in enumerate(d[o]) if x == int(tg[q])), 0)
    es, ed, er, et = idx.search(qv, qi, qc, k, targets=tg)                 # a prune that keeps everything: exact search
    for rate in (1.0, 5.0, 102.4):
        sc, dc, rk, ts, st = idx.search_two_phase(qv, qi, qc, k, "max_ratio", 0.0, rate, targets=tg)
        assert torch.equal(dc, ed) and torch.equal(sc.view(torch.int32), es.view(torch.int32))
        assert torch.equal(ts.view(torch.int32), et.view(torch.int32))
        assert torch.equal(rk, torch.where(er <= k, er, torch.zeros_like(er)))
        assert torch.equal(st["postings_high"], st["postings_all"])


def test_output_is_independent_of_chunking_and_slicing_and_identical_across_runs(dev):
    rng = np.random.default_rng(5)
    V = 500
    docs, queries = _fp32_corpus(rng, 20000, V, 60), _fp32_corpus(rng, 40, V, 30)
    idx = _index(docs, V, dev)
    qv, qi, qc = _to_device(queries, dev)
    tg = torch.tensor(rng.integers(0, len(docs), size=len(queries)), device=dev)
    runs = [idx.search_two_phase(qv, qi, qc, 10, targets=tg, chunk_docs=c, query_slice=s)
            for c, s in ((0, 0), (0, 0), (1000, 0), (32768, 1), (4096, 7))]
    for r in runs[1:]:
        assert torch.equal(r[0].view(torch.int32), runs[0][0].view(torch.int32)) and torch.equal(r[1], runs[0][1])
        assert torch.equal(r[2], runs[0][2]) and torch.equal(r[3].view(torch.int32), runs[0][3].view(torch.int32))
        assert all(torch.equal(r[4][x], runs[0][4][x]) for x in STAT_KEYS)
    C = runs[0][1]
    a = idx.rescore(qv, qi, qc, C, 5, targets=tg)
    b = idx.rescore(qv, qi, qc, C, 5, targets=tg, query_slice=3)
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def test_pruned_index_equals_an_index_of_reference_pruned_rows(dev):
    V = 120
    _, docs, queries, targets = _dyadic_corpus(6, 2000, V, 16)
    idx = _index(docs, V, dev)
    src = [x.clone() for x in (idx.doc_ptr, idx.doc_term, idx.doc_w, idx.term_ptr, idx.post_doc, idx.post_w)]
    qv, qi, qc = _to_device(queries, dev)
    tg = torch.tensor(targets, dtype=torch.int32, device=dev)
    for ptype, value in (("max_ratio", 0.6), ("abs_value", 0.6), ("top_k", 4), ("alpha_mass", 0.7)):
        pruned = idx.pruned(ptype, value)
        want, _ = R.prune(docs, ptype, value)
        assert pruned is not idx and pruned.built and pruned.num_docs == idx.num_docs
        _same_rows((pruned.doc_ptr[1:] - pruned.doc_ptr[:-1], pruned.doc_term, pruned.doc_w), want, (ptype, value))
        assert pruned.nnz == sum(len(t) for t, _ in want) < idx.nnz
        ref = _index(want, V, dev)
        for a, b in zip(pruned.search(qv, qi, qc, 10, targets=tg), ref.search(qv, qi, qc, 10, targets=tg)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (ptype, value)
    assert int((idx.pruned("abs_value", 0.6).doc_ptr[1:] == idx.pruned("abs_value", 0.6).doc_ptr[:-1]).sum()) > \
        int((idx.doc_ptr[1:] == idx.doc_ptr[:-1]).sum())                  # docs pruned to empty stay as empty rows
    now = (idx.doc_ptr, idx.doc_term, idx.doc_w, idx.term_ptr, idx.post_doc, idx.post_w)
    assert all(torch.equal(a, b) for a, b in zip(src, now))                # the source index is untouched
    for bad in (("top_k", 0), ("max_ratio", 2.0), ("nope", 1.0)):
        with pytest.raises(ValueError):
            idx.pruned(*bad)


# ------------------------------------------------------------------------------------------------ evaluator and CLI
def test_two_phase_eval_end_to_end(dev, tmp_path):
    """Plumbing only: a random-init model says nothing about quality."""
    from src.train.data.collator import create_tokenizer
    from src.train.eval import RETRIEVAL_SIZE, MidTrainingEvaluator, two_phase_eval
    tok = create_tokenizer("hash:1000")
    model = _tiny_model(dev, tmp_path)
    kw = dict(tokenizer=tok, val_file=_val_file(tmp_path), max_queries=30, max_docs=90, device=str(dev),
              query_max_length=16, doc_max_length=32, batch_size=16)
    plain = MidTrainingEvaluator(**kw).evaluate(model)
    keep_all = MidTrainingEvaluator(**kw, two_phase={"prune_value": 0.0}).evaluate(model)
    for key, v in plain.items():
        assert keep_all[key] == v, key
    for key in ("recall@1", "recall@5", "recall@10", "mrr@10", "ndcg@10"):
        assert keep_all[f"two_phase_{key}"] == plain[key], key
    assert keep_all["two_phase_overlap@5"] == 1.0 and keep_all["two_phase_postings_frac"] == 1.0
    default = MidTrainingEvaluator(**kw, two_phase={}).evaluate(model)
    extra = {k: v for k, v in default.items() if k.startswith("two_phase_")}
    assert len(extra) == 7 and all(0.0 <= v <= 1.0 for v in extra.values()), extra
    ev = MidTrainingEvaluator(**kw)
    index, queries = ev.encode(model)
    targets = torch.tensor(ev.corpus.targets, dtype=torch.int32, device=dev)
    _, exact_docs, _, _ = index.search(*queries, RETRIEVAL_SIZE, targets=targets)
    m, info = two_phase_eval(index, queries, targets, exact_docs, {}, doc_prune=("top_k", 32))
    assert 0.0 < m["doc_postings_frac"] <= 1.0 and info["index"].nnz <= 32 * index.num_docs
    assert set(m) == set(extra) | {"doc_postings_frac"} and info["search_s"] > 0


def test_cli_sweep_end_to_end(dev, tmp_path, capsys):
    from src.model.splade_modern import SPLADEModernBERT
    from src.train.cli import eval_pruning
    mdir = tmp_path / "model"
    mdir.mkdir()
    (mdir / "config.json").write_text(json.dumps(dict(
        vocab_size=1000, hidden_size=256, intermediate_size=384, num_hidden_layers=2, num_attention_heads=4,
        local_attention=16, pad_token_id=999)))
    torch.manual_seed(5)
    (tmp_path / "ckpt").mkdir()
    torch.save(SPLADEModernBERT(model_name=str(mdir)).state_dict(), tmp_path / "ckpt" / "model.pt")
    argv = ["--checkpoint", str(tmp_path / "ckpt" / "model.pt"), "--model-name", str(mdir), "--tokenizer", "hash:1000",
            "--val-file", _val_file(tmp_path, 80), "--max-queries", "40", "--max-docs", "120", "--query-max-length", "16",
            "--doc-max-length", "32", "--batch-size", "16"]
    one = eval_pruning.main(argv)
    assert len(one) == 1 and (one[0]["prune_value"], one[0]["expansion_rate"], one[0]["max_window_size"]) == (0.4, 5.0, 10000)
    lines = eval_pruning.main(argv + ["--sweep", "--out", str(tmp_path / "sweep.jsonl")])
    printed = [json.loads(x) for x in capsys.readouterr().out.splitlines() if x.startswith("{")]
    assert len(lines) == 19 and printed[1:] == lines
    assert [json.loads(x) for x in open(tmp_path / "sweep.jsonl")] == lines
    fields = {"prune_type", "prune_value", "expansion_rate", "doc_prune_type", "recall@10", "two_phase_recall@10",
              "two_phase_mrr@10", "overlap@5", "postings_high", "postings_all", "window_filled", "search_s"}
    assert all(fields <= set(line) for line in lines)
    assert [line["prune_value"] for line in lines[:5]] == [0.1, 0.2, 0.4, 0.6, 0.8]
    assert [line["doc_prune_type"] for line in lines[10:]] == ["max_ratio"] * 3 + ["top_k"] * 3 + ["alpha_mass"] * 3
    assert all("doc_postings_frac" in line for line in lines[10:]) and lines[2]["two_phase_recall@10"] == \
        one[0]["two_phase_recall@10"]
