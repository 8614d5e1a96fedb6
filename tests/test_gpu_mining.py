"""Hard-negative mining on the GPU: SparseIndex.search_band / pair_scores (csrc/retrieval.hip) and the miner built on them
(src.train.mining, CLI src.train.cli.mine_negatives).

Admissibility (include/snx.h): score > 0, not in the query's exclusion row, score < ceiling (fp32, strict); order score
descending, lowest doc id first; the band is ranks [lo, hi).  With dyadic weights every score is exact in fp32, so the
band must equal a float64 brute force of that definition BIT for BIT."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.test_gpu_retrieval import _dense, _index, _long_query_corpus, _rows, _to_device

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "opensearch-neural-pre-train_amd")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _ref_band(S, lo, hi, excl, ceil):
    nq, nd = S.shape
    w = hi - lo
    docs = np.full((nq, w), -1, np.int64)
    scores = np.zeros((nq, w), np.float64)
    found = np.zeros(nq, np.int64)
    ids = np.arange(nd)
    for q in range(nq):
        s = S[q]
        adm = (s > 0) & ~np.isin(ids, np.asarray(excl[q], np.int64)) & (s < ceil[q])
        order = np.lexsort((ids, -s))
        band = order[adm[order]][lo:hi]
        docs[q, :len(band)] = band
        scores[q, :len(band)] = s[band]
        found[q] = len(band)
    return docs, scores, found


def _band_case(dev, idx, S, queries, lo, hi, excl, ceil=None, chunk_docs=0):
    qv, qi, qc = _to_device(queries, dev, np.random.default_rng(7))
    ct = None if ceil is None else torch.tensor(ceil, dtype=torch.float32, device=dev)
    sc, dc, fd = idx.search_band(qv, qi, qc, lo, hi, exclude=excl, ceiling=ct, chunk_docs=chunk_docs)
    rd, rs, rf = _ref_band(S, lo, hi, excl, np.full(len(queries), np.inf) if ceil is None else np.asarray(ceil))
    assert np.array_equal(dc.cpu().numpy(), rd)
    assert np.array_equal(sc.cpu().numpy().astype(np.float64), rs)
    assert np.array_equal(fd.cpu().numpy(), rf)
    return sc, dc, fd


# ------------------------------------------------------------------------------------------------ exact cases
def test_band_exact_exclusions_ceilings_and_short_bands(dev):
    rng = np.random.default_rng(11)
    V = 40
    docs = _rows(rng, 500, V, 6, np.array([16, 32, 64]), common=7, empty_every=19)
    queries = _rows(rng, 32, V, 5, np.array([16, 32, 64]), empty_every=8)      # queries 0, 8, 16, 24 empty
    queries[5] = (np.array([39]), np.array([1.0]))                              # few nonzero docs: band longer
    idx = _index(docs, V, dev)
    S = _dense(queries, V) @ _dense(docs, V).T
    excl, ceil = [], []
    for q in range(len(queries)):
        order = np.lexsort((np.arange(len(docs)), -S[q]))
        e = list(order[:3]) + list(order[12:15]) + list(rng.choice(len(docs), 4, replace=False))   # above / inside
        excl.append(e)
        pos = int(order[2])
        ceil.append(np.float32(S[q, pos]) if q % 3 == 0 and S[q, pos] > 0 else np.inf)           # hit exactly
    excl[3] = []
    excl[4] = [int(rng.integers(len(docs)))]                                   # a "positive" with no ceiling
    for lo, hi, chunk in ((2, 12, 0), (0, 64, 128), (5, 300, 256)):
        _, _, fd = _band_case(dev, idx, S, queries, lo, hi, excl, ceil, chunk)
        assert fd[0] == 0 and fd[8] == 0
    # equality with the ceiling is not admissible: a ceiling at the top score removes every doc that ties it
    q = 1
    top = np.float32(S[q].max())
    sc, dc, _ = _band_case(dev, idx, S, queries, 0, 10, [[]] * len(queries), [top] * len(queries))
    assert float(sc[q].max()) < top
    # a band longer than the admissible set
    sc, dc, fd = _band_case(dev, idx, S, queries, 0, 64, excl, None, 0)
    assert int(fd[5]) < 64 and (dc[5, int(fd[5]):] == -1).all()
    # one tie run over three chunks (300 = 2 * 128 + 44): every non-empty doc scores 0.25, so rank hi = 140 falls inside
    # the run and inside the second chunk, and the merge takes the tie's first docs across a chunk boundary
    docs = _rows(rng, 300, V, 6, np.array([32]), common=7, empty_every=17)
    queries[5] = (np.array([7]), np.array([0.5]))
    S = _dense(queries, V) @ _dense(docs, V).T
    assert (S[5] > 0).sum() > 256 and np.unique(S[5][S[5] > 0]).size == 1
    _, dc, fd = _band_case(dev, _index(docs, V, dev), S, queries, 5, 140, [[]] * len(queries), None, 128)
    assert int(fd[5]) == 135 and 128 <= int(dc[5, 134]) < 256


@pytest.mark.parametrize("hi", [1, 7])
def test_band_exact_query_longer_than_one_staging_group(dev, hi):
    docs, queries, V = _long_query_corpus()                 # 300 terms in query 0, query 1 empty
    idx = _index(docs, V, dev)
    S = _dense(queries, V) @ _dense(docs, V).T
    excl = [[int(np.argmax(S[0]))], [], [3]]
    _, _, fd = _band_case(dev, idx, S, queries, 0, hi, excl, None, 128)
    assert fd[0] == hi and fd[1] == 0


def test_pair_scores_exact_query_longer_than_one_lookup_step(dev):
    docs, queries, V = _long_query_corpus()                 # 300 terms: five steps of 64 lanes, the last one partial
    idx = _index(docs, V, dev)
    S = _dense(queries, V) @ _dense(docs, V).T
    qv, qi, qc = _to_device(queries, dev, np.random.default_rng(7))
    pq, pd = np.divmod(np.arange(3 * len(docs)), len(docs))
    pairs = torch.from_numpy(np.stack([pq, pd], 1).astype(np.int32)).to(dev)
    ps = idx.pair_scores(qv, qi, qc, pairs)
    assert np.array_equal(ps.cpu().numpy().astype(np.float64), S.reshape(-1))


def test_band_exact_hi_1024_and_100k_docs(dev):
    rng = np.random.default_rng(12)
    V = 64
    docs = _rows(rng, 100_003, V, 12, np.arange(1, 5) * 16, common=3)
    queries = _rows(rng, 24, V, 10, np.arange(1, 5) * 16)
    idx = _index(docs, V, dev)
    S = _dense(queries, V) @ _dense(docs, V).T
    excl = [list(rng.choice(len(docs), 1000, replace=False)) + list(np.argsort(-S[q], kind="stable")[:50])
            for q in range(len(queries))]
    ceil = [np.float32(np.sort(S[q])[-20]) if q % 2 else np.inf for q in range(len(queries))]
    _band_case(dev, idx, S, queries, 1000, 1024, excl, ceil, 256)
    _band_case(dev, idx, S, queries, 0, 1024, excl, ceil, 0)
    _band_case(dev, idx, S, queries, 10, 50, excl, None, 8192)


# ------------------------------------------------------------------------------------------------ agreement
def _random_fp32(rng, n, V, m):
    return [(np.sort(rng.choice(V, size=m, replace=False)),
             rng.uniform(0.01, 3.0, size=m).astype(np.float32).astype(np.float64)) for _ in range(n)]


def test_band_equals_search_with_exclusions_removed(dev):
    rng = np.random.default_rng(13)
    V, nd, nq = 2000, 20000, 40
    docs, queries = _random_fp32(rng, nd, V, 64), _random_fp32(rng, nq, V, 32)
    idx = _index(docs, V, dev)
    qv, qi, qc = _to_device(queries, dev, rng)
    _, top, _, _ = idx.search(qv, qi, qc, 100)
    excl = [sorted(set(top[q, ::7].cpu().tolist()) | set(rng.choice(nd, 30, replace=False).tolist()))
            for q in range(nq)]
    lo, hi = 10, 50
    m = max(len(e) for e in excl)
    sc, dc, _, _ = idx.search(qv, qi, qc, hi + m)
    bs, bd, bf = idx.search_band(qv, qi, qc, lo, hi, exclude=excl)
    sc, dc = sc.cpu().numpy(), dc.cpu().numpy()
    for q in range(nq):
        keep = ~np.isin(dc[q], excl[q]) & (dc[q] >= 0)
        want_d, want_s = dc[q][keep][lo:hi], sc[q][keep][lo:hi]
        assert int(bf[q]) == len(want_d)
        assert np.array_equal(bd[q, :len(want_d)].cpu().numpy(), want_d)
        assert np.array_equal(bs[q, :len(want_d)].cpu().numpy().view(np.int32), want_s.view(np.int32))


def test_pair_scores_equal_search_scores_and_target_score(dev):
    rng = np.random.default_rng(14)
    V, nd, nq = 1500, 8000, 32
    docs, queries = _random_fp32(rng, nd, V, 80), _random_fp32(rng, nq, V, 40)
    idx = _index(docs, V, dev)
    qv, qi, qc = _to_device(queries, dev, rng)
    tg = torch.tensor(rng.integers(0, nd, size=nq), device=dev)
    sc, dc, _, ts = idx.search(qv, qi, qc, 64, targets=tg)
    pairs = torch.stack([torch.arange(nq, device=dev)[:, None].expand(nq, 64).reshape(-1), dc.long().reshape(-1)], 1)
    ps = idx.pair_scores(qv, qi, qc, pairs)
    assert torch.equal(ps.view(torch.int32), sc.reshape(-1).view(torch.int32))
    pt = idx.pair_scores(qv, qi, qc, torch.stack([torch.arange(nq, device=dev), tg], 1))
    assert torch.equal(pt.view(torch.int32), ts.view(torch.int32))


def test_band_is_bit_identical_across_chunk_sizes_and_runs(dev):
    rng = np.random.default_rng(15)
    V, nd, nq = 500, 40000, 48
    docs, queries = _random_fp32(rng, nd, V, 40), _random_fp32(rng, nq, V, 30)
    idx = _index(docs, V, dev)
    qv, qi, qc = _to_device(queries, dev, rng)
    excl = [sorted(rng.choice(nd, 400, replace=False).tolist()) for _ in range(nq)]
    ceil = torch.tensor([np.inf if q % 2 else 40.0 for q in range(nq)], dtype=torch.float32, device=dev)
    runs = [idx.search_band(qv, qi, qc, 5, 200, exclude=excl, ceiling=ceil, chunk_docs=c)
            for c in (0, 0, 256, 4096, 32768)]
    r0 = runs[0]
    assert int(r0[2].min()) > 0
    for r in runs[1:]:
        assert torch.equal(r[0].view(torch.int32), r0[0].view(torch.int32))
        assert torch.equal(r[1], r0[1]) and torch.equal(r[2], r0[2])


# ------------------------------------------------------------------------------------------------ the miner end to end
MODEL_CFG = dict(vocab_size=50000, hidden_size=256, intermediate_size=384, num_hidden_layers=2, num_attention_heads=4,
                 local_attention=16, pad_token_id=49999)
K, LO, HI = 3, 2, 12


def _shards(d):
    from src.train.data import SyntheticTripletDataset
    d.mkdir(parents=True, exist_ok=True)
    a = SyntheticTripletDataset(40, num_negatives=3, seed=21, q_words=(2, 8), d_words=(6, 24))
    b = SyntheticTripletDataset(40, num_negatives=1, seed=22, q_words=(2, 8), d_words=(6, 24))
    ra = [a[i] for i in range(40)]
    rb = [b[i] for i in range(40)]
    for i in range(6):                                         # repeated queries with other positives
        rb[i]["query"] = ra[i]["query"]
    rb[6]["query"] = ra[7]["query"]
    rb[6]["negative"] = ra[7]["positive"]                      # an original negative that is a positive elsewhere
    for i in range(0, 40, 5):
        ra[i].update(pair_type="qd", difficulty="hard", source="syn", teacher_pos_score=0.9,
                     teacher_neg_scores=[0.1, 0.2, 0.3])
    for name, recs in (("train_00.jsonl", ra), ("train_01.jsonl", rb)):
        with open(d / name, "w") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")
    (d / "val.jsonl").write_text(json.dumps(ra[0]) + "\n")
    return ra + rb


def _run_cli(tmp, out, nproc, port, extra=()):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""),
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("SNX_DIST_FORCE", None)
    if nproc > 1:
        env["SNX_DIST_BACKEND"] = "gloo"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc),
           "--master-addr", "127.0.0.1", "--master-port", str(port), "-m", "src.train.cli.mine_negatives",
           "--input-pattern", str(tmp / "data" / "train_*.jsonl"), "--val-pattern", str(tmp / "data" / "val.jsonl"),
           "--output-dir", str(out), "--k", str(K), "--rank-start", str(LO), "--rank-end", str(HI),
           "--checkpoint", str(tmp / "ckpt"), "--model-name", str(tmp / "model"), "--tokenizer", "hash:50000",
           "--query-max-length", "16", "--doc-max-length", "32", "--batch-size", "16", *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=str(tmp))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return r


@pytest.fixture(scope="module")
def mined(dev, tmp_path_factory):
    from src.model.splade_modern import SPLADEModernBERT
    tmp = tmp_path_factory.mktemp("mine")
    (tmp / "model").mkdir()
    (tmp / "model" / "config.json").write_text(json.dumps(MODEL_CFG))
    (tmp / "ckpt").mkdir()
    torch.manual_seed(5)
    model = SPLADEModernBERT(model_name=str(tmp / "model"))
    torch.save(model.state_dict(), tmp / "ckpt" / "model.pt")
    recs = _shards(tmp / "data")
    r1 = _run_cli(tmp, tmp / "out1", 1, 29581)
    r1b = _run_cli(tmp, tmp / "out1b", 1, 29582)
    return tmp, recs, model.to(dev).eval(), (r1, r1b)


def _files(d):
    return {p: (d / p).read_bytes() for p in sorted(os.listdir(d))}


def test_cli_mines_k_admissible_negatives_matching_a_float64_ranking(dev, mined):
    from benchmark.encoders import allowed_token_mask, special_token_ids
    from src.train.data.collator import create_tokenizer
    from src.train.mining import build_corpus, length_batches, token_lengths
    tmp, recs, model, (r1, _) = mined
    out = tmp / "out1"
    assert sorted(os.listdir(out)) == ["train_00.jsonl", "train_01.jsonl", "val.jsonl"]
    assert (out / "val.jsonl").read_bytes() == (tmp / "data" / "val.jsonl").read_bytes()
    assert "MarginMSE is inactive" in r1.stderr + r1.stdout
    c = build_corpus([str(tmp / "data" / "train_00.jsonl"), str(tmp / "data" / "train_01.jsonl")])
    tok = create_tokenizer("hash:50000")
    allowed = allowed_token_mask(tok.convert_ids_to_tokens(list(range(50000))), special_token_ids(tok), 50000).numpy() > 0

    def dense(texts, max_len):
        R = np.zeros((len(texts), 50000))
        for ids in length_batches(token_lengths(tok, texts, max_len), 16):
            enc = tok([texts[i] for i in ids], padding=True, truncation=True, max_length=max_len, return_tensors="pt")
            with torch.no_grad(), torch.autocast(device_type="cuda", dtype=torch.bfloat16):
                rep, _ = model(enc["input_ids"].to(dev), enc["attention_mask"].to(dev))
            R[ids] = rep.float().cpu().numpy().astype(np.float64)
        return np.where((R > 0) & allowed[None, :], R, 0.0)

    D, Q = dense(c.docs, 32), dense(c.queries, 16)
    for row in Q:
        nz = np.flatnonzero(row)
        if len(nz) > 64:
            row[np.setdiff1d(nz, nz[np.lexsort((nz, -row[nz]))[:64]])] = 0.0
    S = Q @ D.T
    doc_id = {t: i for i, t in enumerate(c.docs)}
    got = [json.loads(line) for f in ("train_00.jsonl", "train_01.jsonl") for line in open(out / f)]
    assert len(got) == len(recs) == len(c.records)
    ids = np.arange(len(c.docs))
    for i, g in enumerate(got):
        q = c.rec_query[i]
        assert g["query"] == recs[i]["query"] and g["positive"] == recs[i]["positive"]
        assert len(g["negatives"]) == K and len(g["miner_neg_scores"]) == K
        assert "teacher_pos_score" not in g and "teacher_neg_scores" not in g
        for key in ("pair_type", "difficulty", "source"):
            assert g.get(key) == recs[i].get(key)
        negs = [doc_id[t] for t in g["negatives"]]
        assert not set(negs) & set(c.positives[q])
        s = S[q]
        tol = 1e-5 * max(s.max(), 1e-30)
        assert abs(g["miner_pos_score"] - s[c.rec_pos[i]]) <= tol
        order = np.lexsort((ids, -s))
        adm = order[(s[order] > 0) & ~np.isin(order, c.positives[q])][LO:HI]
        assert len(adm) >= K
        for j, d in enumerate(negs):
            assert abs(g["miner_neg_scores"][j] - s[d]) <= tol
            assert abs(s[d] - s[adm[j]]) <= 2 * tol           # a swap only between float64 near-ties


def test_cli_output_is_byte_identical_across_runs(mined):
    tmp = mined[0]
    assert _files(tmp / "out1") == _files(tmp / "out1b")


def test_cli_two_ranks_match_one_rank_byte_for_byte(mined):
    tmp = mined[0]
    _run_cli(tmp, tmp / "out2", 2, 29583)
    assert _files(tmp / "out2") == _files(tmp / "out1")


def test_mined_shard_trains_one_micro_step(dev, mined, tmp_path):
    from src.model.losses import SPLADELossV33
    from src.model.splade_modern import SPLADEModernBERT
    from src.train.core import ddp_trainer as T
    from src.train.data import TripletCollator, load_training_data
    from src.train.data.collator import create_tokenizer
    tmp = mined[0]
    ds = load_training_data([str(tmp / "out1" / "train_*.jsonl")])
    col = TripletCollator(create_tokenizer("hash:50000"), query_max_length=16, doc_max_length=32)
    batch = col([ds[i] for i in range(4)])
    assert batch["num_negatives"] == K
    assert tuple(batch["negative_input_ids"].shape[:1]) == (4 * K,)
    torch.manual_seed(5)
    model = SPLADEModernBERT(model_name=str(tmp / "model")).to(dev)
    model.train()
    loss_fn = SPLADELossV33(temperature=20.0, flops_warmup_steps=4).to(dev)
    loss, _ = T.micro_step(model, loss_fn, batch, 0, dev, 1, last_of_window=True)
    assert torch.isfinite(loss)


def test_cli_self_teacher_scores_and_ceiling(dev, mined):
    from src.train.mining import record_negatives
    tmp = mined[0]
    _run_cli(tmp, tmp / "out3", 1, 29584, ("--teacher-scores", "self", "--max-score-ratio", "0.9",
                                             "--sample", "random", "--seed", "3"))
    got = [json.loads(line) for line in open(tmp / "out3" / "train_00.jsonl")]
    src = [json.loads(line) for line in open(tmp / "data" / "train_00.jsonl")]
    mined_recs = 0
    for g, r in zip(got, src):
        assert len(g["negatives"]) == K
        assert g["teacher_pos_score"] == g["miner_pos_score"]
        assert g["teacher_neg_scores"] == g["miner_neg_scores"]
        if set(g["negatives"]) <= set(record_negatives(r)):
            continue                                           # an empty band: the record's own negatives
        mined_recs += 1
        # ceiling = fp32(0.9) * min over the query's positives <= fp32(0.9) * this positive's score, strict
        assert all(np.float32(s) < np.float32(0.9) * np.float32(g["miner_pos_score"]) for s in g["miner_neg_scores"])
    assert mined_recs > len(got) // 2
