"""Exact sparse retrieval on the GPU (csrc/retrieval.hip via snx.retrieval.SparseIndex) and the mid-training evaluator
built on it (src.train.eval.MidTrainingEvaluator, CLI wiring of ref:src/train/cli/train_v33_ddp.py:629-644,679-697).

Score definition (include/snx.h): fmaf over the shared terms in ascending term id.  With dyadic weights (multiples of
2^-6 below 4) every product and partial sum is exact in fp32, so scores, top-k lists and target ranks must equal a numpy
reference BIT for BIT, ties included (score descending, lowest doc id first)."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "opensearch-neural-pre-train_amd")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ helpers
def _rows(rng, n, V, max_nnz, levels, common=None, empty_every=0):
    """n sparse rows: (terms sorted, weights) lists; weights are `levels` * 2^-6.  `common`: a term in every row."""
    out = []
    for i in range(n):
        if empty_every and i % empty_every == 0:
            out.append((np.zeros(0, np.int64), np.zeros(0, np.float64)))
            continue
        m = int(rng.integers(1, max_nnz + 1))
        t = rng.choice(V, size=m, replace=False)
        if common is not None and common not in t:
            t[0] = common
        t = np.sort(t)
        w = rng.choice(levels, size=m).astype(np.float64) / 64.0
        out.append((t, w))
    return out


def _to_device(rows, dev, shuffle_rng=None):
    """rows -> ([n, cap] fp32 values, [n, cap] int32 ids, [n] int32 counts), entries optionally shuffled in a row (as
    ops.sparse_topk's weight-ordered output is)."""
    n = len(rows)
    cap = max([1] + [len(t) for t, _ in rows])
    vals = np.zeros((n, cap), np.float32)
    ids = np.zeros((n, cap), np.int32)
    cnt = np.zeros(n, np.int32)
    for i, (t, w) in enumerate(rows):
        p = shuffle_rng.permutation(len(t)) if shuffle_rng is not None else np.arange(len(t))
        vals[i, :len(t)] = w[p]
        ids[i, :len(t)] = t[p]
        cnt[i] = len(t)
    return (torch.from_numpy(vals).to(dev), torch.from_numpy(ids).to(dev), torch.from_numpy(cnt).to(dev))


def _dense(rows, V):
    D = np.zeros((len(rows), V), np.float64)
    for i, (t, w) in enumerate(rows):
        D[i, t] = w
    return D


def _index(docs, V, dev, batch=4096):
    from snx.retrieval import SparseIndex
    idx = SparseIndex(V, dev)
    for s in range(0, len(docs), batch):
        idx.add(*_to_device(docs[s:s + batch], dev))
    return idx.build()


def _ref_rank(S, k, targets):
    """float64 scores [nq, nd] -> top-k docs / scores (score > 0, desc, lowest id first) and target ranks."""
    nq, nd = S.shape
    docs = np.full((nq, k), -1, np.int64)
    scores = np.zeros((nq, k), np.float64)
    ranks = np.zeros(nq, np.int64)
    ids = np.arange(nd)
    for q in range(nq):
        s = S[q]
        order = np.lexsort((ids, -s))
        order = order[s[order] > 0][:k]
        docs[q, :len(order)] = order
        scores[q, :len(order)] = s[order]
        if targets is not None:
            t = targets[q]
            st = s[t]
            ranks[q] = 0 if st == 0 else 1 + int((s > st).sum()) + int(((s == st) & (ids < t)).sum())
    return docs, scores, ranks


def _search_exact_case(dev, docs, queries, V, k, targets, chunk_docs=0):
    idx = _index(docs, V, dev)
    qv, qi, qc = _to_device(queries, dev, np.random.default_rng(5))
    tg = torch.tensor(targets, dtype=torch.int32, device=dev)
    sc, dc, rk, ts = idx.search(qv, qi, qc, k, targets=tg, chunk_docs=chunk_docs)
    S = _dense(queries, V) @ _dense(docs, V).T
    rd, rs, rr = _ref_rank(S, k, np.asarray(targets))
    assert np.array_equal(dc.cpu().numpy(), rd)
    assert np.array_equal(sc.cpu().numpy().astype(np.float64), rs)
    assert np.array_equal(rk.cpu().numpy(), rr)
    assert np.array_equal(ts.cpu().numpy().astype(np.float64), S[np.arange(len(queries)), targets])
    return idx, S, rr


# ------------------------------------------------------------------------------------------------ exact cases
def test_exact_small_with_empty_rows_common_term_and_short_lists(dev):
    rng = np.random.default_rng(1)
    V = 40
    docs = _rows(rng, 300, V, 6, np.array([16, 32, 64]), common=7, empty_every=17)     # doc 0, 17, ... empty
    queries = _rows(rng, 40, V, 5, np.array([16, 32, 64]), empty_every=9)                # query 0, 9, ... empty
    queries[5] = (np.array([7]), np.array([0.5]))                # only the term in every non-empty doc: all ties
    queries[6] = (np.array([39]), np.array([1.0]))               # a rare term: fewer nonzero docs than k
    targets = [int(rng.integers(0, 300)) for _ in queries]
    targets[1] = 0                                               # an empty doc: score 0, a miss
    _, S, rr = _search_exact_case(dev, docs, queries, V, 64, targets, chunk_docs=128)   # 300 = 2 * 128 + 44
    assert rr[0] == 0 and rr[1] == 0 and rr[9] == 0
    assert (S[6] > 0).sum() < 64                                 # k larger than the nonzero-score docs
    assert (S > 0).any(axis=1).sum() > 20


def test_exact_many_chunks_100k_docs(dev):
    rng = np.random.default_rng(2)
    V = 64
    docs = _rows(rng, 100_003, V, 12, np.arange(1, 5) * 16, common=3)
    queries = _rows(rng, 48, V, 10, np.arange(1, 5) * 16)
    targets = [int(rng.integers(0, len(docs))) for _ in queries]
    for k, chunk in ((10, 0), (1024, 32768), (100, 8192)):       # 7, 4 and 13 chunks, last one partial
        _search_exact_case(dev, docs, queries, V, k, targets, chunk_docs=chunk)


def _long_query_corpus():
    """V = 1024, 300 docs, 3 queries: one of 300 terms (more than the 256 terms whose chunk bounds are staged at once and
    more than the 64 a pair-score step looks up, so those loops run twice and more), one empty, one ordinary."""
    rng = np.random.default_rng(23)
    V = 1024
    docs = _rows(rng, 300, V, 40, np.array([16, 32, 64]), common=7, empty_every=17)
    queries = _rows(rng, 3, V, 12, np.array([16, 32, 64]))
    t = np.sort(rng.choice(V, size=300, replace=False))
    queries[0] = (t, rng.choice(np.array([16, 32, 64]), size=300).astype(np.float64) / 64.0)
    queries[1] = (np.zeros(0, np.int64), np.zeros(0, np.float64))
    return docs, queries, V


@pytest.mark.parametrize("k", [1, 7])
def test_exact_query_longer_than_one_staging_group(dev, k):
    docs, queries, V = _long_query_corpus()
    _, S, rr = _search_exact_case(dev, docs, queries, V, k, [5, 9, 0], chunk_docs=128)   # target 0: an empty doc
    assert (S[0] > 0).sum() > 7 and rr[0] > 0 and rr[1] == 0 and rr[2] == 0


# ------------------------------------------------------------------------------------------------ fp32 rounding
def test_random_fp32_within_bound_of_float64(dev):
    rng = np.random.default_rng(3)
    V, nd, nq, k = 2000, 10000, 64, 100
    docs, queries = [], []
    for n, out, m in ((nd, docs, 128), (nq, queries, 64)):
        for _ in range(n):
            t = np.sort(rng.choice(V, size=m, replace=False))
            out.append((t, rng.uniform(0.01, 3.0, size=m).astype(np.float32).astype(np.float64)))
    targets = rng.integers(0, nd, size=nq)
    idx = _index(docs, V, dev)
    qv, qi, qc = _to_device(queries, dev, rng)
    sc, dc, rk, ts = idx.search(qv, qi, qc, k, targets=torch.tensor(targets, device=dev))
    S = _dense(queries, V) @ _dense(docs, V).T                  # all terms positive: sum|q_w d_w| = S
    tol = 1e-6 * S
    sc, dc, rk, ts = sc.cpu().numpy(), dc.cpu().numpy(), rk.cpu().numpy(), ts.cpu().numpy()
    exact_ranks = 0
    for q in range(nq):
        s = S[q]
        assert np.all(np.abs(sc[q] - s[dc[q]]) <= tol[q][dc[q]])
        assert np.all(np.diff(sc[q]) <= 0)
        rest = np.setdiff1d(np.arange(nd), dc[q])
        assert s[rest].max() <= sc[q].min() + 2 * tol[q].max()
        t = targets[q]
        assert abs(ts[q] - s[t]) <= tol[q][t]
        lo = 1 + int((s > s[t] + 2 * tol[q][t]).sum())
        hi = 1 + int((s > s[t] - 2 * tol[q][t]).sum()) - 1
        assert lo <= rk[q] <= hi
        if lo >= hi:
            exact_ranks += 1
            assert rk[q] == lo
        ref_order = np.lexsort((np.arange(nd), -s))[:k]
        gaps = np.abs(np.diff(s[ref_order]))
        if np.all(gaps > 2 * tol[q][ref_order].max()):
            assert np.array_equal(dc[q], ref_order)
    assert exact_ranks > nq // 2


# ------------------------------------------------------------------------------------------------ determinism
def test_index_and_search_are_bit_reproducible(dev):
    rng = np.random.default_rng(4)
    V = 500
    docs = [(np.sort(rng.choice(V, size=int(rng.integers(1, 80)), replace=False)), None) for _ in range(30000)]
    docs = [(t, rng.uniform(0.01, 2.0, size=len(t)).astype(np.float32).astype(np.float64)) for t, _ in docs]
    queries = [(np.sort(rng.choice(V, size=40, replace=False)), rng.uniform(0.01, 2.0, size=40)) for _ in range(50)]
    a, b = _index(docs, V, dev, batch=7000), _index(docs, V, dev, batch=3000)
    for x, y in ((a.term_ptr, b.term_ptr), (a.post_doc, b.post_doc), (a.post_w.view(torch.int32), b.post_w.view(torch.int32))):
        assert torch.equal(x, y)
    # the postings are the doc CSR transposed, each list in doc order
    tp = a.term_ptr.cpu().numpy()
    pd = a.post_doc.cpu().numpy()
    assert tp[-1] == sum(len(t) for t, _ in docs)
    assert all(np.all(np.diff(pd[tp[v]:tp[v + 1]]) > 0) for v in range(V))
    qv, qi, qc = _to_device(queries, dev, rng)
    tg = torch.tensor(rng.integers(0, len(docs), size=50), device=dev)
    runs = [a.search(qv, qi, qc, 200, targets=tg, chunk_docs=c) for c in (0, 0, 1000, 4096, 32768)]
    runs.append(b.search(qv, qi, qc, 200, targets=tg))
    r0 = runs[0]
    for r in runs[1:]:
        assert torch.equal(r[0].view(torch.int32), r0[0].view(torch.int32))
        assert torch.equal(r[1], r0[1]) and torch.equal(r[2], r0[2])
        assert torch.equal(r[3].view(torch.int32), r0[3].view(torch.int32))


# ------------------------------------------------------------------------------------------------ evaluator
def _tiny_model(dev, tmp_path, seed=0):
    from src.model.splade_modern import SPLADEModernBERT
    mdir = tmp_path / "model"
    mdir.mkdir(exist_ok=True)
    (mdir / "config.json").write_text(json.dumps(dict(
        vocab_size=1000, hidden_size=256, intermediate_size=384, num_hidden_layers=2, num_attention_heads=4,
        local_attention=16, pad_token_id=999)))
    torch.manual_seed(seed)
    return SPLADEModernBERT(model_name=str(mdir)).to(dev)


def _val_file(tmp_path, n=60):
    from src.train.data import SyntheticTripletDataset
    ds = SyntheticTripletDataset(n, num_negatives=2, seed=11, q_words=(2, 8), d_words=(6, 24))
    p = tmp_path / "val.jsonl"
    with open(p, "w") as f:
        for i in range(n):
            f.write(json.dumps(ds[i]) + "\n")
    return str(p)


def test_evaluate_equals_float64_ranking_of_the_dense_representations(dev, tmp_path):
    from benchmark.encoders import allowed_token_mask, special_token_ids
    from src.train.data.collator import create_tokenizer
    from src.train.eval import QUERY_TOP_K, MidTrainingEvaluator, metrics_from_ranks
    tok = create_tokenizer("hash:1000")
    model = _tiny_model(dev, tmp_path)
    model.train()
    ev = MidTrainingEvaluator(tokenizer=tok, val_file=_val_file(tmp_path), max_queries=30, max_docs=90,
                              device=str(dev), query_max_length=16, doc_max_length=32, batch_size=16)
    m = ev.evaluate(model)
    assert model.training                                         # the previous mode is restored
    c = ev.corpus
    allowed = allowed_token_mask(tok.convert_ids_to_tokens(list(range(1000))), special_token_ids(tok), 1000).numpy() > 0

    def dense(texts, max_len):
        out = []
        with torch.no_grad():
            model.eval()
            for s in range(0, len(texts), 16):
                enc = tok(texts[s:s + 16], padding=True, truncation=True, max_length=max_len, return_tensors="pt")
                rep, _ = model(enc["input_ids"].to(dev), enc["attention_mask"].to(dev))
                out.append(rep.float().cpu().numpy().astype(np.float64))
            model.train()
        R = np.concatenate(out)
        return np.where((R > 0) & allowed[None, :], R, 0.0)

    D = dense(c.docs, 32)
    Q = dense(c.queries, 16)
    for row in Q:                                                  # top 64 by weight, ties lowest id first
        nz = np.flatnonzero(row)
        if len(nz) > QUERY_TOP_K:
            keep = nz[np.lexsort((nz, -row[nz]))[:QUERY_TOP_K]]
            drop = np.setdiff1d(nz, keep)
            row[drop] = 0.0
    S = Q @ D.T
    ids = np.arange(len(c.docs))
    ranks = []
    for q, t in enumerate(c.targets):
        s, st = S[q], S[q, t]
        r = 0 if st == 0 else 1 + int((s > st).sum()) + int(((s == st) & (ids < t)).sum())
        near = np.abs(s - st) <= 1e-5 * max(st, 1e-30)
        near[t] = False
        ranks.append(ev.last_ranks[q] if near.any() else r)      # a float64 near-tie: fp32 decides, either is right
    want = metrics_from_ranks(ranks)
    for key in ("recall@1", "recall@5", "recall@10", "mrr@10", "ndcg@10"):
        assert m[key] == want[key], (key, m[key], want[key])
    assert m["num_queries"] == 30 and m["num_docs"] == len(c.docs)
    assert m["avg_nnz_d"] == pytest.approx((D > 0).sum(1).mean())
    assert m["avg_nnz_q"] == pytest.approx((Q > 0).sum(1).mean())
    assert 0 < m["avg_nnz_q"] <= QUERY_TOP_K


def test_evaluation_between_steps_leaves_training_bit_identical(dev, tmp_path, monkeypatch):
    """SNX_DET_REDUCE=1 (default): 2 optimizer steps, evaluate, 2 more == 4 steps without the evaluation, bit for bit."""
    from oracle import splade_oracle as O
    from src.model.losses import SPLADELossV33
    from src.train.config.v33 import V33Config
    from src.train.core import ddp_trainer as T
    from src.train.data.collator import create_tokenizer
    from src.train.eval import MidTrainingEvaluator
    monkeypatch.delenv("SNX_DET_REDUCE", raising=False)
    cfg = O.EncoderConfig(vocab_size=1000, hidden_size=256, intermediate_size=384, num_hidden_layers=2,
                          num_attention_heads=4, local_attention=16, pad_token_id=999)
    gen = torch.Generator().manual_seed(5)
    batches = [O.synth_batch(4, 16, 32, cfg, gen, k=1, ragged=True) for _ in range(4)]
    conf = V33Config()
    conf.training.gradient_accumulation_steps = 1
    conf.training.learning_rate = 1e-3
    ev = MidTrainingEvaluator(tokenizer=create_tokenizer("hash:1000"), val_file=_val_file(tmp_path, 30),
                              max_queries=12, max_docs=40, device=str(dev), query_max_length=16, doc_max_length=32)

    def run(with_eval):
        model = _tiny_model(dev, tmp_path, seed=3)
        model.train()
        loss_fn = SPLADELossV33(temperature=20.0, flops_warmup_steps=4).to(dev)
        opt = T.build_optimizer(model, conf)
        sch = T.build_scheduler(opt, 0, 4)
        losses = []
        for i, b in enumerate(batches):
            if with_eval and i == 2:
                metrics = ev.evaluate(model)
                assert metrics["num_queries"] == 12
            loss, _ = T.micro_step(model, loss_fn, b, i, dev, 1, last_of_window=True)
            losses.append(float(loss))
            T.optimizer_step(model, opt, sch, conf)
        torch.cuda.synchronize()
        return losses, {n: p.detach().clone() for n, p in model.named_parameters()}

    l0, p0 = run(False)
    l1, p1 = run(True)
    assert l0 == l1
    for n in p0:
        assert torch.equal(p0[n], p1[n]), n


def test_cli_logs_mid_training_eval_under_torchrun(dev, tmp_path):
    import subprocess
    import sys
    import yaml
    mdir = tmp_path / "model"
    mdir.mkdir()
    (mdir / "config.json").write_text(json.dumps(dict(
        vocab_size=1000, hidden_size=256, intermediate_size=384, num_hidden_layers=2, num_attention_heads=4,
        local_attention=16, pad_token_id=999)))
    out = tmp_path / "out"
    cfg = {"model": {"name": str(mdir)},
           "loss": {"temperature": 20.0, "flops_warmup_steps": 4},
           "data": {"train_files": ["synthetic:8"], "val_files": ["synthetic:24:2"], "batch_size": 4,
                    "query_max_length": 16, "doc_max_length": 32, "num_workers": 0},
           "training": {"num_epochs": 5, "gradient_accumulation_steps": 1, "output_dir": str(out),
                        "log_every_n_steps": 1, "save_every_n_epochs": 5, "learning_rate": 1e-3}}
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(cfg))
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""),
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("SNX_DIST_FORCE", None)
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1",
                        "--master-addr", "127.0.0.1", "--master-port", "29561", "-m", "src.train.cli.train_v33_ddp",
                        "--config", str(tmp_path / "cfg.yaml"), "--tokenizer", "hash:1000"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    log = (out / "training.log").read_text()
    assert "Mid-training evaluator initialized" in log, log[-3000:]
    assert "Eval epoch 5: R@1=" in log, log[-3000:]
    assert "Eval failed" not in log and "Training complete" in log
