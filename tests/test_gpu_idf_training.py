"""GPU checks of IDF-aware training and the doc-only query mode at the trainer's level: ddp_trainer.micro_step with
SPLADELossIDF on the tiny geometry, and the doc_only method of the benchmark CLI.  Restatement: tests/idf_reference.py and
float64 torch."""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import idf_reference as R

pytestmark = pytest.mark.gpu
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g14_benchmark_dir")
U = 2.0 ** -24
BASE_KEYS = {"infonce", "flops_q", "flops_d", "flops_neg", "lambda_q", "lambda_d", "lambda_neg", "kd", "margin_mse",
             "nonzero_q", "nonzero_d"}
NEW_KEYS = {"idf_flops_q", "idf_flops_d", "idf_flops_neg"}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def tiny():
    """(cfg, params, batch, penalty weights, query idf, allowed): built once, never modified."""
    from oracle import splade_oracle as O
    from snx.idf import penalty_weights
    from tests.test_gpu_no_token_weights import _tiny_cfg
    cfg = _tiny_cfg()
    params = O.perturb_params(O.init_params(cfg, seed=3), seed=4, scale=2.0, bias_mean=-0.1)
    batch = O.synth_batch(4, 24, 70, cfg, torch.Generator().manual_seed(77), k=1, ragged=True)
    rng = np.random.default_rng(8)
    V = cfg.vocab_size
    idf = (rng.random(V) * 6 + 0.3).astype(np.float32)
    w = penalty_weights(idf, special_ids=[0, 1, V - 1], stopword_ids=[10, 11])
    allowed = np.ones(V, dtype=np.uint8)
    allowed[[0, 1, V - 1]] = 0
    return cfg, params, batch, w, torch.from_numpy(idf), torch.from_numpy(allowed)


def _loss(tiny, dev, doc_only, w=None, **kw):
    from src.model.losses import SPLADELossIDF
    _, _, _, pw, idf, allowed = tiny
    args = dict(lambda_q=0.01, lambda_d=0.004, temperature=20.0, flops_warmup_steps=4)
    args.update(kw)
    return SPLADELossIDF(penalty_weights=pw if w is None else w, beta=0.3, query_idf=idf if doc_only else None,
                         query_allowed=allowed if doc_only else None, **args).to(dev)


def _spy(monkeypatch):
    """Every (input_ids) batch that reaches the encoder and every pooled output it returns: model(...) and
    model.forward_many(...) both arrive at EncoderRuntime.forward_many."""
    from snx.encoder import EncoderRuntime
    real = EncoderRuntime.forward_many
    seen, reps = [], []

    def spy(self, pairs, lengths=None, need_token_weights=True):
        out = real(self, pairs, lengths, need_token_weights=need_token_weights)
        for (ids, _), (rep, _) in zip(pairs, out):
            seen.append(ids.detach().cpu())
            reps.append(rep)
        return out
    monkeypatch.setattr(EncoderRuntime, "forward_many", spy)
    return seen, reps


@pytest.mark.parametrize("fused", [True, False], ids=["forward_many", "two_calls"])
def test_doc_only_micro_step_encodes_no_query_and_equals_the_restatement(dev, tiny, monkeypatch, fused):
    """fp32 mode (SNX_PRECISION=fp32: encoder and loss outside autocast), so that the InfoNCE term is the one the loss
    kernels are held to golden g4 on (tests/test_gpu_model.py::test_loss_kernels_vs_golden_g4: rel 2e-5)."""
    from src.train.core import ddp_trainer as T
    from tests.test_gpu_model import _build_model
    cfg, params, batch, w, idf, allowed = tiny
    monkeypatch.setenv("SNX_FUSED_PASSES", "1" if fused else "0")
    monkeypatch.setenv("SNX_PRECISION", "fp32")
    seen, reps = _spy(monkeypatch)
    model = _build_model(cfg, params, dev)
    model.train()
    loss_fn = _loss(tiny, dev, doc_only=True)
    step = 2
    loss, d = T.micro_step(model, loss_fn, batch, step, dev, 1)
    torch.cuda.synchronize()
    # exactly two passes, neither over the query's ids
    assert len(seen) == 2
    q_ids = batch["query_input_ids"]
    assert not any(s.shape == q_ids.shape and torch.equal(s, q_ids) for s in seen)
    assert torch.equal(seen[0], batch["positive_input_ids"]) and torch.equal(seen[1], batch["negative_input_ids"])
    assert set(d) == BASE_KEYS | NEW_KEYS and d["lambda_q"] == 0.0
    # the restatement, float64, on the fp32 reps the passes returned
    p32, n32 = (r.detach().float().cpu().numpy() for r in reps)
    q32 = R.query_dense(batch["query_input_ids"].numpy(), batch["query_attention_mask"].numpy(), allowed.numpy(),
                        idf.numpy())
    q, p, n = (torch.from_numpy(x).double() for x in (q32, p32, n32))
    sc = torch.cat([q @ p.T, (q * n).sum(1, keepdim=True)], 1) / 20.0
    infonce = float((torch.logsumexp(sc, 1) - sc.diagonal()).mean())
    lam_d, lam_n = d["lambda_d"], d["lambda_neg"]
    want, bound = infonce, 2e-5 * abs(infonce)                 # the g4 tolerance of the InfoNCE term
    for lam, x, key in ((lam_d, p32, "idf_flops_d"), (lam_n, n32, "idf_flops_neg")):
        s1, s2, P, a1, a2 = R.penalty(R.column_means_fp32(x), w.numpy(), 0.3)
        pb = R.penalty_bound(cfg.vocab_size, a1 + float(np.float32(0.3)) * a2, P)
        assert abs(float(d[key]) - P) <= pb
        l32 = float(np.float32(lam))
        want += l32 * P
        bound += l32 * pb + U * abs(l32 * P)                   # P's bound, the fp32 product lambda * P ...
        bound += U * abs(want)                                 # ... and the fp32 sum that adds it to the loss
    print(f"loss={float(loss)!r} want={want!r} err={abs(float(loss) - want):.3e} bound={bound:.3e}")
    assert abs(float(loss) - want) <= bound
    # nonzero_q counts the IDF rows' entries
    assert float(d["nonzero_q"]) == pytest.approx(float((q32 > 0).sum()) / q32.shape[0], rel=1e-6)
    grads = [prm.grad for prm in model.parameters()]
    assert all(g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in grads)


@pytest.mark.parametrize("fused", [True, False], ids=["forward_many", "two_calls"])
def test_doc_only_step_is_reproducible_and_repeats(dev, tiny, monkeypatch, fused):
    """bf16 (the training configuration): the same step from the same state gives the same gradient bits under the ordered
    reductions (det_reduce = 1, the default), and a second step runs -- on the unfused path through the micro-step arena,
    which then holds two passes instead of three."""
    import snx
    from src.train.core import ddp_trainer as T
    from tests.test_gpu_model import _build_model
    cfg, params, batch, *_ = tiny
    monkeypatch.setenv("SNX_FUSED_PASSES", "1" if fused else "0")
    monkeypatch.delenv("SNX_PRECISION", raising=False)
    assert snx.config("det_reduce") == 1
    out = []
    for _ in range(2):
        model = _build_model(cfg, params, dev)
        model.train()
        loss_fn = _loss(tiny, dev, doc_only=True)
        loss, _ = T.micro_step(model, loss_fn, batch, 2, dev, 1)
        out.append((loss.clone(), [prm.grad.clone() for prm in model.parameters()]))
    assert torch.equal(out[0][0], out[1][0])
    assert all(torch.equal(a, b) for a, b in zip(out[0][1], out[1][1]))
    assert all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in out[0][1])
    model.zero_grad(set_to_none=True)
    seen, _ = _spy(monkeypatch)
    for _ in range(2):
        loss, _ = T.micro_step(model, loss_fn, batch, 3, dev, 1)
    assert len(seen) == 4 and bool(torch.isfinite(loss))
    assert all(bool(torch.isfinite(prm.grad).all()) for prm in model.parameters())


@pytest.mark.parametrize("fused", [True, False], ids=["forward_many", "three_calls"])
def test_encoder_mode_runs_three_passes_and_zero_weights_equal_the_base_loss(dev, tiny, monkeypatch, fused):
    from src.model.losses import SPLADELossV33
    from src.train.core import ddp_trainer as T
    from tests.test_gpu_model import _build_model
    cfg, params, batch, w, *_ = tiny
    monkeypatch.setenv("SNX_FUSED_PASSES", "1" if fused else "0")
    monkeypatch.delenv("SNX_PRECISION", raising=False)
    seen, _ = _spy(monkeypatch)
    model = _build_model(cfg, params, dev)
    model.train()
    loss, d = T.micro_step(model, _loss(tiny, dev, doc_only=False), batch, 2, dev, 1)
    assert len(seen) == 3 and torch.equal(seen[0], batch["query_input_ids"])
    assert set(d) == BASE_KEYS | NEW_KEYS
    assert d["lambda_q"] > 0 and float(d["idf_flops_q"]) > 0 and float(d["idf_flops_d"]) > 0 and float(d["idf_flops_neg"]) > 0
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(prm.grad).all()) for prm in model.parameters())
    # penalty weights of zero: the loss and every parameter gradient are those of SPLADELossV33 with all lambda = 0
    got, ref = [], []
    for store, fn in ((got, _loss(tiny, dev, doc_only=False, w=torch.zeros_like(w))),
                      (ref, SPLADELossV33(lambda_q=0.0, lambda_d=0.0, temperature=20.0, flops_warmup_steps=4).to(dev))):
        m = _build_model(cfg, params, dev)
        m.train()
        ls, dd = T.micro_step(m, fn, batch, 2, dev, 1)
        store.extend([ls.clone(), [prm.grad.clone() for prm in m.parameters()], dd])
    assert torch.equal(got[0], ref[0])
    assert all(torch.equal(a, b) for a, b in zip(got[1], ref[1]))
    for key in ("infonce", "flops_q", "flops_d", "flops_neg", "nonzero_q", "nonzero_d"):
        assert float(got[2][key]) == float(ref[2][key]), key       # flops_* stay the base kernel's unweighted values


def test_mid_training_evaluator_with_query_idf(dev, tiny):
    """Doc-only evaluation: the query rows are IDF rows, whatever the model is; the documents are the model's."""
    from src.train.data.collator import create_tokenizer
    from src.train.eval import MidTrainingEvaluator
    from tests.test_gpu_model import _build_model
    cfg, params, *_ = tiny
    tok = create_tokenizer(f"hash:{cfg.vocab_size}")
    rng = np.random.default_rng(2)
    idf = torch.from_numpy((rng.random(cfg.vocab_size) * 5 + 0.2).astype(np.float32))
    model = _build_model(cfg, params, dev)
    ev = MidTrainingEvaluator(tok, "synthetic:24", max_queries=8, max_docs=40, device=str(dev), query_max_length=16,
                              doc_max_length=32, batch_size=5, query_idf=idf)
    index, queries = ev.encode(model)
    enc = tok(ev.corpus.queries, padding=True, truncation=True, max_length=16, return_tensors="pt")
    want = R.query_rows(enc["input_ids"].numpy(), enc["attention_mask"].numpy(),
                        ev._allowed_mask(cfg.vocab_size).cpu().numpy(), idf.numpy())
    vals, ids, cnt = (x.cpu().numpy() for x in queries)
    for r, (terms, ws) in enumerate(want):
        assert cnt[r] == len(terms) and ids[r, :cnt[r]].tolist() == terms
        assert np.array_equal(vals[r, :cnt[r]], np.asarray(ws, dtype=np.float32))
    m = ev.evaluate(model)
    assert m["num_queries"] == 8 and 0.0 <= m["recall@1"] <= m["recall@10"] <= 1.0
    assert m["avg_nnz_q"] == pytest.approx(float(cnt.mean()))


def test_compute_idf_end_to_end(dev, tmp_path, capsys):
    """The CLI on two small shards with the hash tokenizer: counts against Python sets over the same tokenisation (no
    special tokens, no truncation), the files in the exchange format, one JSON line."""
    from snx.idf import load_idf
    from src.train.cli import compute_idf as Cc
    from src.train.data.collator import create_tokenizer
    rng = np.random.default_rng(3)
    words = [f"t{i}" for i in range(40)]
    texts = []
    for s in range(2):
        with open(tmp_path / f"train_shard_{s}.jsonl", "w") as f:
            for _ in range(30):
                rec = {"query": " ".join(rng.choice(words, 5)), "positive": " ".join(rng.choice(words, 90)),
                       "negative": "", "other": "ignored"}
                f.write(json.dumps(rec) + "\n")
                texts += [rec["query"], rec["positive"]]
            f.write("\n{broken\n")
    line = Cc.main(["--input", str(tmp_path / "train_shard_*.jsonl"), "--output", str(tmp_path / "out" / "idf"),
                    "--tokenizer", "hash:500", "--smoothing", "smooth", "--batch-docs", "16", "--pt",
                    "--idf-json", str(tmp_path / "idf.json")])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == line
    tok = create_tokenizer("hash:500")
    df = [0] * 500
    for t in texts:
        for i in set(tok.encode(t, add_special_tokens=False)):
            df[i] += 1
    want = R.idf(df, len(texts), "smooth")
    got, meta = load_idf(tmp_path / "out" / "idf")
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert meta == {"vocab_size": 500, "num_docs": 120, "smoothing": "smooth", "tokenizer_name": "hash:500",
                    "dtype": "float32", "byte_order": "little_endian"}
    assert line == {"num_docs": 120, "vocab_size": 500, "nonzero": 500, "min": float(want.min()), "max": float(want.max())}
    assert torch.equal(torch.load(tmp_path / "out" / "idf.pt"), torch.from_numpy(want))
    assert len(json.load(open(tmp_path / "idf.json"))) == 500


def test_eval_benchmark_doc_only(dev, tmp_path, capsys):
    from snx.idf import save_idf
    from src.model.splade_modern import SPLADEModernBERT
    from src.train.cli import eval_benchmark as E
    from src.train.cli.mine_negatives import load_model
    from src.train.data.collator import create_tokenizer
    from src.train.eval import BenchmarkEvaluator, load_benchmark_dir
    mdir = tmp_path / "model"
    mdir.mkdir()
    (mdir / "config.json").write_text(json.dumps(dict(
        vocab_size=1000, hidden_size=256, intermediate_size=384, num_hidden_layers=2, num_attention_heads=4,
        local_attention=16, pad_token_id=999)))
    torch.manual_seed(5)
    (tmp_path / "ckpt").mkdir()
    torch.save(SPLADEModernBERT(model_name=str(mdir)).state_dict(), tmp_path / "ckpt" / "model.pt")
    rng = np.random.default_rng(14)
    idf = (rng.random(1000) * 7 + 0.1).astype(np.float32)
    save_idf(tmp_path / "idf", idf, 12, "bm25", "hash:1000")
    argv = ["--checkpoint", str(tmp_path / "ckpt" / "model.pt"), "--model-name", str(mdir), "--tokenizer", "hash:1000",
            "--benchmark-dir", GOLDEN_DIR, "--query-max-length", "16", "--doc-max-length", "32", "--batch-size", "8",
            "--bootstrap", "0", "--methods", "sparse,doc_only", "--idf", str(tmp_path / "idf")]
    lines = E.main(argv)
    printed = [json.loads(x) for x in capsys.readouterr().out.splitlines() if x.startswith("{")]
    assert printed == json.loads(json.dumps(lines))
    assert [x.get("method", x.get("test")) for x in lines] == ["sparse", "doc_only", "sparse_vs_doc_only"]
    line = lines[1]
    assert set(line) == set(lines[0]) - {"first_relevant"}
    # the restatement: IDF rows against the same document index, float64 scores, ties lowest doc id first
    tok = create_tokenizer("hash:1000")
    data = load_benchmark_dir(GOLDEN_DIR)
    ev = BenchmarkEvaluator(tok, data, device=str(dev), query_max_length=16, doc_max_length=32, batch_size=8)
    index, _ = ev.encode(load_model(E.parse_args(argv), dev))
    ptr, term, wt = (x.cpu().numpy() for x in (index.doc_ptr, index.doc_term, index.doc_w))
    docs = np.zeros((index.num_docs, 1000), dtype=np.float32)
    for dno in range(index.num_docs):
        docs[dno, term[ptr[dno]:ptr[dno + 1]]] = wt[ptr[dno]:ptr[dno + 1]]
    enc = tok(data.queries, padding=True, truncation=True, max_length=16, return_tensors="pt")
    rows = R.query_rows(enc["input_ids"].numpy(), enc["attention_mask"].numpy(), ev._allowed_mask(1000).cpu().numpy(), idf)
    sc = R.scores(rows, docs)
    vals = np.zeros((len(rows), 5))
    for qi in range(len(rows)):
        order = sorted((dno for dno in range(index.num_docs) if sc[qi, dno] > 0), key=lambda dno: (-sc[qi, dno], dno))[:10]
        s = [sc[qi, dno] for dno in order]
        assert all(a - b > 1e-5 * a for a, b in zip(s[:-1], s[1:]))            # no near-tie a fp32 score could turn
        first = next((i + 1 for i, dno in enumerate(order) if dno in data.relevant[qi]), None)
        if first is not None:
            vals[qi] = [first <= 1, first <= 5, first <= 10, 1.0 / first, 1.0 / math.log2(first + 1)]
    for key, col in (("recall@1", 0), ("recall@5", 1), ("recall@10", 2), ("mrr", 3), ("ndcg@10", 4)):
        assert line[key] == pytest.approx(float(vals[:, col].mean()), abs=1e-12), key
    assert line["num_queries"] == 7 and line["num_docs"] == 12
