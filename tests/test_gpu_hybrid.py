"""GPU checks of the BM25 baseline and rank fusion (csrc/hybrid.hip, include/snx.h "BM25 baseline and rank fusion")
against the numpy references tests/bm25_reference.py and tests/fusion_reference.py, which the host suite
(test_hybrid_host.py) pins by hand and holds to the reference project's own outputs (tests/golden/g13_fusion.json).
Everything is compared exactly: integers, fp32 bits, float64 bits."""
import json
import os

import numpy as np
import pytest
import torch

from tests import bm25_reference as B
from tests import fusion_reference as F
from tests.test_gpu_retrieval import _tiny_model, _val_file
from tests.test_hybrid_host import golden_fusion, runs_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _bits(a):
    a = np.asarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _tokens(rng, n, S, V, special=()):
    """Token rows with repeats (a Zipf-like draw), ragged masks, and the given special rows."""
    ids = np.minimum(rng.zipf(1.3, (n, S)) - 1, V - 1).astype(np.int64)
    lens = rng.integers(0, S + 1, n)
    mask = (np.arange(S)[None, :] < lens[:, None]).astype(np.int64)
    for r, kind in enumerate(special):
        if r >= n:
            break
        if kind == "masked":
            mask[r] = 0
        elif kind == "repeated":
            ids[r], mask[r] = 7, 1
        elif kind == "outside":
            ids[r, ::2], mask[r] = -3, 1
            ids[r, 1::4] = V + 5
        elif kind == "full":
            mask[r] = 1
        elif kind == "holes":
            mask[r] = rng.integers(0, 2, S) * 5                  # any non-zero value counts
    return ids, mask


def _allowed(rng, V):
    a = (rng.random(V) > 0.2).astype(np.uint8)
    a[7] = 1
    return a


# ------------------------------------------------------------------------------------------------ term counts
def test_term_counts_equal_the_reference(dev):
    from snx.retrieval import term_counts, term_counts_max_len
    smax = term_counts_max_len()
    assert smax == 8192
    rng = np.random.default_rng(0)
    V = 5000
    allowed = _allowed(rng, V)
    special = ("masked", "repeated", "outside", "full", "holes")
    for S, n in ((1, 300), (64, 3000), (256, 600), (512, 300), (smax, 24)):
        ids, mask = _tokens(rng, n, S, V, special)
        got = term_counts(torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev), torch.from_numpy(allowed).to(dev))
        want = B.term_counts(ids, mask, allowed)
        for g, w, what in zip(got, want, ("term", "tf", "cnt", "len")):
            assert g.dtype == torch.int32 and np.array_equal(g.cpu().numpy(), w), (S, what)
        assert np.array_equal(want[1].sum(1), want[3])
    with pytest.raises(ValueError):
        z = torch.zeros((2, smax + 1), dtype=torch.long, device=dev)
        term_counts(z, z, torch.from_numpy(allowed).to(dev))


# ------------------------------------------------------------------------------------------------ df, weights, index
def _bm25(dev, ids, mask, allowed, batches, k1=1.2, b=0.75):
    from snx.retrieval import Bm25Index
    bm = Bm25Index(len(allowed), dev, k1=k1, b=b)
    al = torch.from_numpy(allowed).to(dev)
    s = 0
    for m in batches:
        bm.add_tokens(torch.from_numpy(ids[s:s + m]).to(dev), torch.from_numpy(mask[s:s + m]).to(dev), al)
        s += m
    assert s == len(ids)
    return bm.build()


def test_doc_freq_accumulates_exactly_over_unequal_batches(dev):
    rng = np.random.default_rng(1)
    V, S, n = 800, 96, 1000
    allowed = _allowed(rng, V)
    ids, mask = _tokens(rng, n, S, V, ("masked", "repeated", "outside"))
    bm = _bm25(dev, ids, mask, allowed, (1, 300, 57, 642))
    rows, df, dl, idf, avg = B.bm25_rows(ids, mask, allowed)
    assert np.array_equal(bm.doc_freq.cpu().numpy(), df) and bm.doc_freq.dtype == torch.int32
    assert np.array_equal(bm.doc_len.cpu().numpy(), dl) and bm.avgdl == avg
    assert np.array_equal(_bits(bm.idf.cpu().numpy()), _bits(idf))
    tp = bm.index.term_ptr.cpu().numpy()
    assert np.array_equal(tp[1:] - tp[:-1], df)                    # the built index's posting-list lengths


def test_bm25_weights_equal_the_reference_bit_for_bit(dev):
    rng = np.random.default_rng(2)
    V, S, n = 600, 128, 700
    allowed = np.ones(V, np.uint8)
    ids, mask = _tokens(rng, n, S, V, ("holes", "repeated", "full"))
    ids[ids == V - 1] = 0
    ids[5, 1], mask[5, 1] = V - 1, 1                               # df = 1 for the last term
    ids[:, 0], mask[:, 0] = 7, 1                                   # df = N for term 7 (no doc is empty here)
    ids[1], mask[1] = 7, 1                                         # tf = S
    for k1, b in ((1.2, 0.75), (1.2, 0.0), (1.2, 1.0), (0.0, 0.75), (2.0, 0.3)):
        bm = _bm25(dev, ids, mask, allowed, (n,), k1, b)
        rows, df, dl, idf, avg = B.bm25_rows(ids, mask, allowed, k1, b)
        assert df[7] == n and df[V - 1] == 1 and rows[1][0].tolist() == [7] and dl[1] == S
        want_w = np.concatenate([w for _, w in rows])
        want_t = np.concatenate([t for t, _ in rows])
        assert np.array_equal(bm.index.doc_term.cpu().numpy(), want_t), (k1, b)
        assert np.array_equal(_bits(bm.index.doc_w.cpu().numpy()), _bits(want_w)), (k1, b)
        assert (want_w > 0).all()


def test_search_tokens_equals_search_over_reference_weights(dev):
    from snx.retrieval import SeismicIndex, SparseIndex
    from tests.test_gpu_retrieval import _to_device
    rng = np.random.default_rng(3)
    V, n, nq = 400, 900, 120
    allowed = _allowed(rng, V)
    ids, mask = _tokens(rng, n, 80, V, ("masked", "repeated", "outside"))
    qids, qmask = _tokens(rng, nq, 12, V, ("masked", "repeated"))
    bm = _bm25(dev, ids, mask, allowed, (400, 500))
    rows = B.bm25_rows(ids, mask, allowed)[0]
    ref = SparseIndex(V, dev)
    cnt = torch.tensor([len(t) for t, _ in rows], dtype=torch.long, device=dev)
    ref.add_csr(cnt, torch.from_numpy(np.concatenate([t for t, _ in rows]).astype(np.int32)).to(dev),
                torch.from_numpy(np.concatenate([w for _, w in rows])).to(dev))
    ref.build()
    targets = torch.from_numpy(rng.integers(0, n, nq).astype(np.int32)).to(dev)
    al = torch.from_numpy(allowed).to(dev)
    got = bm.search_tokens(torch.from_numpy(qids).to(dev), torch.from_numpy(qmask).to(dev), al, 10, targets=targets)
    qrows = [(t, w.astype(np.float32)) for t, w in B.query_rows(qids, qmask, allowed)]
    want = ref.search(*_to_device(qrows, dev), 10, targets=targets)
    for g, w, what in zip(got, want, ("scores", "docs", "rank", "tscore")):
        assert np.array_equal(_bits(g.cpu().numpy()), _bits(w.cpu().numpy())), what
    assert int((got[1] >= 0).sum()) > nq                            # it finds things
    q = bm.query_rows(torch.from_numpy(qids).to(dev), torch.from_numpy(qmask).to(dev), al)
    _, d2, _, _, _ = bm.index.search_two_phase(*q, 10)
    _, d3, _, _, _ = SeismicIndex(bm.index).search(*q, 10)
    assert int((d2 >= 0).sum()) > 0 and int((d3 >= 0).sum()) > 0
    # every doc empty: an index that finds nothing
    empty = _bm25(dev, ids[:5], np.zeros_like(mask[:5]), allowed, (5,))
    assert empty.avgdl == 0.0 and empty.index.nnz == 0
    s, d, r, _ = empty.search_tokens(torch.from_numpy(qids).to(dev), torch.from_numpy(qmask).to(dev), al, 5,
                                     targets=torch.zeros(nq, dtype=torch.int32, device=dev))
    assert bool((d == -1).all()) and bool((s == 0).all()) and bool((r == 0).all())


# ------------------------------------------------------------------------------------------------ fusion
def _stack(lists, R, dev):
    """One query's lists -> the (docs [1, R], scores [1, R]) pairs fuse_ranked takes."""
    out = []
    for d, s in lists:
        dd, ss = np.full((1, R), -1, np.int32), np.zeros((1, R), np.float32)
        dd[0, :len(d)], ss[0, :len(s)] = d, s
        out.append((torch.from_numpy(dd).to(dev), torch.from_numpy(ss).to(dev)))
    return out


def test_fuse_ranked_reproduces_the_reference_project_bit_for_bit(dev):
    from snx.retrieval import fuse_ranked
    n = 0
    for case in golden_fusion()["fusion"]:
        lists = [(c["docs"], c["scores"]) for c in case["lists"]]
        R = max([1] + [len(d) for d, _ in lists])
        for run, want in runs_of(case):
            od, osc = F.fuse(lists, run["method"], **run["params"])
            for tgt in ([int(od[len(od) // 2])] if len(od) else []) + [10 ** 6]:
                sc, dc, rk, tot = fuse_ranked(_stack(lists, R, dev), run["method"], max(1, len(want)),
                                              targets=torch.tensor([tgt], device=dev), **run["params"])
                assert int(tot[0]) == run["total_hits"] == len(want), case["name"]
                got = {int(d): float(s) for d, s in zip(dc[0].tolist(), sc[0].tolist()) if d >= 0}
                assert {d: s.hex() for d, s in got.items()} == {d: s.hex() for d, s in want.items()}, (case["name"], run)
                assert dc[0].tolist()[:len(od)] == od.tolist(), (case["name"], run)            # order as defined
                assert int(rk[0]) == (od.tolist().index(tgt) + 1 if tgt in od.tolist() else 0)
                n += 1
    assert n > 100


def _random_lists(rng, L, nq, R, nd):
    docs = np.full((L, nq, R), -1, np.int32)
    scores = np.zeros((L, nq, R), np.float32)
    for l in range(L):
        for q in range(nq):
            m = int(rng.integers(0, R + 1)) if q % 7 else (R if q % 14 else 0)
            m = min(m, nd)
            docs[l, q, :m] = rng.choice(nd, m, replace=False)
            scores[l, q, :m] = np.sort(rng.integers(1, 64, m).astype(np.float32) / 8)[::-1]
            if m < R:
                docs[l, q, m + 1:] = rng.integers(0, nd, R - m - 1)            # behind the end marker: not part of the list
    return docs, scores


@pytest.mark.parametrize("R", [10, 100, 1000, 1024])
def test_fuse_ranked_at_scale_equals_the_reference(dev, R):
    from snx.retrieval import fuse_ranked
    rng = np.random.default_rng(R)
    nq = 2000
    for L in (2, 3, 4):
        docs, scores = _random_lists(rng, L, nq, R, nd=max(R + R // 2, 16))       # heavy overlap between the lists
        targets = rng.integers(0, max(R + R // 2, 16), nq).astype(np.int32)
        lists = [(torch.from_numpy(docs[l]).to(dev), torch.from_numpy(scores[l]).to(dev)) for l in range(L)]
        methods = [("rrf", {"k": 60}), ("weighted_rrf", {"k": 20, "weights": [0.4, 0.6, 1.5, 0.25][:L]})]
        if L == 2:
            methods += [("linear", {"alpha": 0.4}), ("linear", {"alpha": 1.0})]
        for top_k in (10, min(4096, L * R)):
            for method, params in methods:
                got = fuse_ranked(lists, method, top_k, targets=torch.from_numpy(targets).to(dev), **params)
                want = F.fuse_batch(docs, scores, method, top_k, targets, **params)
                for g, w, what in zip(got, want, ("scores", "docs", "rank", "total")):
                    assert np.array_equal(_bits(g.cpu().numpy()), _bits(w)), (R, L, method, top_k, what)
                if top_k == 10:
                    break                                                         # one method at the small top_k


# ------------------------------------------------------------------------------------------------ evaluator and CLI
def test_evaluator_hybrid_keys_equal_the_direct_searches(dev, tmp_path):
    """Plumbing only: a random-init model says nothing about quality."""
    from snx.retrieval import fuse_ranked
    from src.train.data.collator import create_tokenizer
    from src.train.eval import (HYBRID_KEYS, RETRIEVAL_SIZE, MidTrainingEvaluator, bm25_index, hybrid_params,
                                metrics_from_ranks, paired_t_test)
    tok = create_tokenizer("hash:1000")
    model = _tiny_model(dev, tmp_path)
    kw = dict(tokenizer=tok, val_file=_val_file(tmp_path), max_queries=30, max_docs=90, device=str(dev),
              query_max_length=16, doc_max_length=32, batch_size=16)
    plain = MidTrainingEvaluator(**kw).evaluate(model)
    assert list(MidTrainingEvaluator(**kw, hybrid=None).evaluate(model)) == list(plain)
    ev = MidTrainingEvaluator(**kw, hybrid={})
    out = ev.evaluate(model)
    assert list(out) == list(plain) + list(HYBRID_KEYS)
    for key, v in plain.items():
        assert out[key] == v, key
    first = ev._bm25[0]
    assert ev.evaluate(model) == out and ev._bm25[0] is first      # the BM25 index is built once per evaluator
    index, queries = ev.encode(model)
    targets = torch.tensor(ev.corpus.targets, dtype=torch.int32, device=dev)
    p = hybrid_params({})
    bm, bq = bm25_index(ev, index.V, p)
    b_s, b_d, b_rank, _ = bm.index.search(*bq, 100, targets=targets)
    s_s, s_d, s_rank, _ = index.search(*queries, 100, targets=targets)
    _, _, h_rank, total = fuse_ranked([(b_d, b_s), (s_d, s_s)], "rrf", RETRIEVAL_SIZE, targets=targets, k=60)
    b_rank, s_rank, h_rank = b_rank.cpu().tolist(), s_rank.cpu().tolist(), h_rank.cpu().tolist()
    for key, v in metrics_from_ranks(b_rank).items():
        assert out[f"bm25_{key}"] == v, key
    for key, v in metrics_from_ranks(h_rank).items():
        assert out[f"hybrid_{key}"] == v, key
    assert out["hybrid_total"] == float(total.double().mean()) and out["hybrid_total"] >= 1.0
    same = lambda a, b: a == b or (a != a and b != b)                          # noqa: E731
    assert same(out["sparse_vs_bm25_p"], paired_t_test(s_rank, b_rank)["p_value"])
    assert same(out["hybrid_vs_sparse_p"], paired_t_test(h_rank, s_rank)["p_value"])
    assert sum(1 for r in b_rank if r) > 0                                      # BM25 finds targets on lexical overlap


def test_cli_prints_parseable_rows(dev, tmp_path, capsys):
    from src.model.splade_modern import SPLADEModernBERT
    from src.train.cli import eval_hybrid
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
    base = eval_hybrid.main(argv)
    assert [x["method"] for x in base] == ["sparse", "bm25", "bm25_sparse_rrf"]
    rng = np.random.default_rng(0)
    nd = base[0]["num_docs"]
    dense = np.stack([rng.permutation(nd)[:50] for _ in range(40)])
    np.savez(tmp_path / "dense.npz", docs=dense, scores=np.sort(rng.random((40, 50)), 1)[:, ::-1])
    lines = eval_hybrid.main(argv + ["--sweep", "--dense-run", str(tmp_path / "dense.npz"), "--out", str(tmp_path / "h.jsonl")])
    printed = [json.loads(x) for x in capsys.readouterr().out.splitlines() if x.startswith("{")]
    assert len(lines) == 11 and printed[3:] == json.loads(json.dumps(lines))
    assert [json.loads(x) for x in open(tmp_path / "h.jsonl")] == printed[3:]
    assert [x["method"] for x in lines] == ["sparse", "bm25", "bm25_sparse_rrf", "bm25_sparse_linear_0.3",
                                           "bm25_sparse_linear_0.4", "bm25_sparse_linear_0.5", "bm25_sparse_weighted_rrf",
                                           "dense", "bm25_dense_rrf", "dense_sparse_rrf", "triple_rrf"]
    fields = {"recall@1", "recall@10", "mrr@10", "ndcg@10", "vs_bm25_p", "vs_bm25_statistic", "vs_bm25_significant"}
    assert all(fields <= set(x) for x in lines) and lines[1]["vs_bm25_p"] is None
    assert lines[:3] == base and all("total" in x for x in lines if x["fusion"])
    assert lines[-1]["retrievers"] == ["bm25", "dense", "sparse"] and lines[-1]["total"] >= lines[2]["total"]
