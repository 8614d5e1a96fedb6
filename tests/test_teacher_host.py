"""Dense teacher encoder without a GPU: ``forward_torch`` against the transformers golden (tests/golden/g21_teacher, written
by tools/make_golden_teacher.py), the position rule, ``from_pretrained``, the reference API (src.model.teachers) on the CPU
fallback, and the ``teacher_scores encode`` CLI."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import dense_reference as R
from tests import teacher_helpers as TH


def _cpu_encoder(precision="fp32"):
    from snx.teacher import TeacherEncoder
    _, cfg, sd = TH.golden()
    return TeacherEncoder(cfg, sd, "cpu", precision)


def _write_model_dir(path, cfg, sd, prefix="", pooling=None):
    os.makedirs(path, exist_ok=True)
    hf = {"model_type": "xlm-roberta", "hidden_act": "gelu", **{k: getattr(cfg, k) for k in cfg.__dataclass_fields__}}
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(hf, f)
    torch.save({prefix + k: v for k, v in sd.items()}, os.path.join(path, "pytorch_model.bin"))
    if pooling is not None:
        os.makedirs(os.path.join(path, "1_Pooling"), exist_ok=True)
        with open(os.path.join(path, "1_Pooling", "config.json"), "w") as f:
            json.dump(pooling, f)
    return str(path)


def test_imports_need_no_gpu():
    import snx.teacher  # noqa: F401
    import src.model
    import src.model.teachers  # noqa: F401
    assert not hasattr(src.model, "BGEM3Teacher")                  # the package does not import the teachers eagerly


def test_recipe_hashes_match_the_golden():
    from snx.teacher import hf_parameter_order, random_state_dict
    g, cfg, _ = TH.golden()
    sd = random_state_dict(cfg, g["seed"])
    assert list(g["sha256"]) == hf_parameter_order(cfg)
    assert {k: TH.sha(v) for k, v in sd.items()} == g["sha256"]


@pytest.mark.parametrize("call", ("batch", "single"))
def test_forward_torch_fp32_against_the_golden(call):
    from snx.teacher import forward_torch
    g, cfg, sd = TH.golden()
    ids, mask, gcls, gemb, e32, _, e_ref = TH.golden_reference(call)
    cls, emb = forward_torch(cfg, sd, ids, mask)
    assert torch.equal(emb, e32)
    assert float((emb - gemb).abs().max()) <= 1e-5
    assert bool(((cls - gcls).abs().amax(dim=1) <= 1e-5 * gcls.abs().amax(dim=1)).all())
    assert 1e-4 < e_ref < 1e-2                                     # the emulated-bf16 mode rounds, and only rounds
    if call == "batch":
        assert [len(s) for s in g["calls"][call]["sequences"]] == [2, 3, 17, 64, 65, 130, 257]
        assert all(s[0] == 0 and s[-1] == 2 for s in g["calls"][call]["sequences"])
        assert g["calls"][call]["max_offdiag_cosine"] < 0.99


def test_padded_call_equals_one_sequence_at_a_time():
    from snx.teacher import forward_torch
    g, cfg, sd = TH.golden()
    ids, mask, _, _, emb = TH.golden_reference("batch")[:5]
    for i, s in enumerate(g["calls"]["batch"]["sequences"]):
        _, one = forward_torch(cfg, sd, *TH.pad_batch([s]))
        assert float((one[0] - emb[i]).abs().max()) <= 1e-6, i


def test_position_ids_rule():
    from snx.teacher import position_ids
    mask = torch.tensor([[1, 1, 1, 0, 0], [1, 1, 1, 1, 1], [0, 0, 1, 1, 0]])
    assert position_ids(mask, 1).tolist() == [[2, 3, 4, 1, 1], [2, 3, 4, 5, 6], [1, 1, 2, 3, 1]]
    transformers = pytest.importorskip("transformers")
    emb = transformers.models.xlm_roberta.modeling_xlm_roberta.XLMRobertaEmbeddings
    ids = torch.where(mask == 1, torch.full_like(mask, 7), torch.ones_like(mask))
    assert torch.equal(emb.create_position_ids_from_input_ids(ids, 1), position_ids(mask, 1))


def test_encode_tokens_rejects_bad_batches():
    enc = _cpu_encoder()
    ids = torch.zeros(2, 4, dtype=torch.long)
    with pytest.raises(ValueError, match="all zero"):
        enc.encode_tokens(ids, torch.tensor([[1, 1, 0, 0], [0, 0, 0, 0]]))
    with pytest.raises(ValueError, match="max_position_embeddings"):
        enc.encode_tokens(torch.zeros(1, 299, dtype=torch.long), torch.ones(1, 299, dtype=torch.long))
    with pytest.raises(ValueError, match="input_ids"):
        enc.encode_tokens(torch.full((1, 4), 300), torch.ones(1, 4, dtype=torch.long))
    with pytest.raises(ValueError):
        enc.encode_tokens(ids, torch.ones(2, 5, dtype=torch.long))
    enc.encode_tokens(torch.zeros(1, 298, dtype=torch.long), torch.ones(1, 298, dtype=torch.long))   # position 299: the last row


@pytest.mark.parametrize("prefix", ("", "roberta."))
def test_from_pretrained_round_trip_through_transformers(tmp_path, prefix):
    transformers = pytest.importorskip("transformers")
    from snx.teacher import TeacherEncoder, random_state_dict
    g, cfg, sd = TH.golden()
    hf_cfg = transformers.XLMRobertaConfig(hidden_act="gelu", **g["config"])
    if prefix:
        model = transformers.XLMRobertaForMaskedLM(hf_cfg)         # keys carry "roberta.", and there is an lm_head
        model.roberta.load_state_dict(random_state_dict(cfg, g["seed"]), strict=False)
    else:
        model = transformers.XLMRobertaModel(hf_cfg, add_pooling_layer=True)          # pooler keys are ignored
        model.load_state_dict(random_state_dict(cfg, g["seed"]), strict=False)
    model.save_pretrained(str(tmp_path / "m"))
    with open(tmp_path / "m" / "config.json") as f:
        assert json.load(f)["model_type"] == "xlm-roberta"
    enc = TeacherEncoder.from_pretrained(str(tmp_path / "m"), device="cpu", precision="fp32")
    assert all(torch.equal(enc.params[k], sd[k]) for k in sd)
    ids, mask, _, gemb = TH.golden_reference("single")[:4]
    assert float((enc.encode_tokens(ids, mask) - gemb).abs().max()) <= 1e-5


def test_from_pretrained_reads_a_plain_directory_and_checks_pooling(tmp_path):
    from snx.teacher import TeacherEncoder
    _, cfg, sd = TH.golden()
    cls_pool = {"word_embedding_dimension": 256, "pooling_mode_cls_token": True, "pooling_mode_mean_tokens": False}
    d = _write_model_dir(tmp_path / "ok", cfg, sd, prefix="roberta.", pooling=cls_pool)
    enc = TeacherEncoder.from_pretrained(d, device="cpu", precision="fp32")
    assert all(torch.equal(enc.params[k], sd[k]) for k in sd)
    mean_pool = {"word_embedding_dimension": 256, "pooling_mode_cls_token": False, "pooling_mode_mean_tokens": True}
    with pytest.raises(ValueError, match="CLS pooling"):
        TeacherEncoder.from_pretrained(_write_model_dir(tmp_path / "mean", cfg, sd, pooling=mean_pool), device="cpu")
    with pytest.raises(FileNotFoundError, match="never resolved"):
        TeacherEncoder.from_pretrained("BAAI/bge-m3", device="cpu")
    bad = _write_model_dir(tmp_path / "bert", cfg, sd)
    with open(os.path.join(bad, "config.json"), "w") as f:
        json.dump({"model_type": "bert"}, f)
    with pytest.raises(ValueError, match="xlm-roberta"):
        TeacherEncoder.from_pretrained(bad, device="cpu")
    short = dict(sd)
    del short["encoder.layer.1.output.dense.bias"]
    with pytest.raises(KeyError):
        TeacherEncoder.from_pretrained(_write_model_dir(tmp_path / "short", cfg, short), device="cpu")


def test_encode_sorts_packs_and_restores_the_input_order():
    enc = _cpu_encoder()
    tok = TH.ToyTokenizer(300)
    calls = []
    inner = enc.encode_tokens
    enc.encode_tokens = lambda ids, mask, normalize=True: (calls.append(int(mask.sum())), inner(ids, mask, normalize))[1]
    small = enc.encode(TH.TEXTS, tok, max_length=256, batch_tokens=130)
    assert len(calls) > 1 and all(c <= 130 for c in calls)
    large = enc.encode(TH.TEXTS, tok, max_length=256)
    assert float((small - large).abs().max()) <= 1e-6
    for i, t in enumerate(TH.TEXTS):
        assert float((enc.encode([t], tok, max_length=256)[0] - large[i]).abs().max()) <= 1e-6, i
    assert enc.encode([], tok).shape == (0, 256)
    assert len(tok(TH.TEXTS[10], max_length=16)["input_ids"][0]) == 16


def test_bge_m3_teacher_methods_on_the_cpu_fallback(tmp_path):
    from src.model.teachers import BGEM3Teacher, KDLossWithBGEM3, create_bge_m3_teacher
    _, cfg, sd = TH.golden()
    tok = TH.ToyTokenizer(300)
    d = _write_model_dir(tmp_path / "m", cfg, sd)
    t = BGEM3Teacher(d, device="cpu", max_length=64, tokenizer=tok, precision="fp32")
    assert isinstance(create_bge_m3_teacher(d, device="cpu", max_length=32, tokenizer=tok), BGEM3Teacher)
    q, docs = TH.TEXTS[:4], TH.TEXTS[4:8]
    eq, ed = t.encode(q), t.encode(docs)
    direct = _cpu_encoder().encode(q, tok, max_length=64)
    assert torch.equal(eq, direct) and eq.shape == (4, 256)
    assert float((eq.norm(dim=-1) - 1).abs().max()) <= 1e-6
    assert t.encode(q[0]).shape == (1, 256)                        # a single string is one text
    sim = eq @ ed.t()
    assert float((t.compute_similarity(eq, ed) - sim).abs().max()) <= 1e-6
    assert float((t.get_ranking_scores(q, docs) - sim.diag()).abs().max()) <= 1e-6
    soft, raw = t.get_soft_labels(q[0], docs[0], docs[1:], temperature=2.0)
    assert float((raw - sim[0]).abs().max()) <= 1e-6 and float((soft - F.softmax(sim[0] / 2.0, -1)).abs().max()) <= 1e-6
    negs = [[docs[(i + 1) % 4], docs[(i + 2) % 4]] for i in range(4)]
    soft, raw = t.get_batch_soft_labels(q, docs, negs, temperature=3.0)
    want = torch.stack([sim[i, [i, (i + 1) % 4, (i + 2) % 4]] for i in range(4)])
    assert raw.shape == (4, 3) and float((raw - want).abs().max()) <= 1e-6
    assert float((soft - F.softmax(want / 3.0, -1)).abs().max()) <= 1e-6
    per_query = torch.stack([t.get_soft_labels(q[i], docs[i], negs[i], temperature=3.0)[0] for i in range(4)])
    assert float((soft - per_query).abs().max()) <= 1e-6           # one encode call for all documents: the same values
    inb = t.get_in_batch_soft_labels(q, docs, temperature=2.0)
    assert float((inb - F.softmax(sim / 2.0, -1)).abs().max()) <= 1e-6
    assert t.to("cpu") is t and t.device == "cpu"
    raw_t = BGEM3Teacher(d, device="cpu", max_length=64, normalize_embeddings=False, tokenizer=tok, precision="fp32")
    e = raw_t.encode(q)
    assert float((F.normalize(e, dim=-1) - eq).abs().max()) <= 1e-6 and float((e.norm(dim=-1) - 1).abs().min()) > 1e-3
    student = torch.randn(4, 4, generator=torch.Generator().manual_seed(1), requires_grad=True)
    out = KDLossWithBGEM3(t, kl_weight=1.0, mse_weight=0.5, temperature=2.0)(student, q, docs)
    kl = F.kl_div(F.log_softmax(student / 2.0, -1), F.softmax(sim / 2.0, -1), reduction="batchmean")
    mse = F.mse_loss(student, sim)
    assert float((out["kl"] - kl).detach().abs()) <= 1e-6 and float((out["mse"] - mse).detach().abs()) <= 1e-6
    assert float((out["total"] - (4.0 * kl + 0.5 * mse)).detach().abs()) <= 1e-5
    out["total"].backward()
    assert student.grad is not None and bool(torch.isfinite(student.grad).all())


def _shards(tmp_path):
    T = TH.TEXTS
    recs = {"train_000.jsonl": [{"query": T[0], "positive": T[1], "negative": T[2]},
                                 {"query": T[3], "positive": T[4], "negatives": [T[5], T[2], T[8]]},
                                 "this line is not json",
                                 {"query": T[0], "positive": T[1]}],
            "train_001.jsonl": [{"query": T[6], "positive": T[7], "negative": T[8], "negatives": [T[9], None]},
                                 {"query": T[9], "positive": T[10], "negative": None}]}
    os.makedirs(tmp_path / "data", exist_ok=True)
    for name, rows in recs.items():
        with open(tmp_path / "data" / name, "w", encoding="utf-8") as f:
            for r in rows:
                f.write((r if isinstance(r, str) else json.dumps(r, ensure_ascii=False)) + "\n")
    return str(tmp_path / "data" / "train_*.jsonl"), [T[i] for i in (0, 1, 2, 3, 4, 5, 8, 6, 7, 9, 10)]


def test_cli_encode_writes_the_cache_score_reads(tmp_path):
    from src.train.cli import teacher_scores
    from src.train.mining.dense import load_teacher_cache, text_hash, write_teacher_scores
    _, cfg, sd = TH.golden()
    tok = TH.ToyTokenizer(300)
    model = _write_model_dir(tmp_path / "m", cfg, sd)
    pattern, order = _shards(tmp_path)
    base = ["encode", "--model-dir", model, "--input-pattern", pattern, "--device", "cpu", "--precision", "fp32",
            "--max-length", "64", "--batch-tokens", "130"]
    assert teacher_scores.main(base + ["--output-dir", str(tmp_path / "one")], tokenizer=tok) == (11, 11)
    emb, tix = load_teacher_cache(str(tmp_path / "one" / "embeddings.npy"), str(tmp_path / "one" / "text_index.json"))
    assert emb.dtype == np.float32 and emb.shape == (11, 256)
    assert tix == {text_hash(t): i for i, t in enumerate(order)}   # first-occurrence order, duplicates once
    direct = _cpu_encoder().encode(order, tok, max_length=64).numpy()
    assert float(np.abs(np.asarray(emb) - direct).max()) <= 1e-6
    rows = 0
    for i in range(3):                                             # three processes, then the merge
        rows += teacher_scores.main(base + ["--output-dir", str(tmp_path / "three"), "--num-shards", "3", "--shard-index",
                                            str(i)], tokenizer=tok)[1]
    assert rows == 11 and not os.path.exists(tmp_path / "three" / "embeddings.npy")
    assert teacher_scores.main(["encode", "--merge", "--output-dir", str(tmp_path / "three")]) == 11
    merged, tix3 = load_teacher_cache(str(tmp_path / "three" / "embeddings.npy"), str(tmp_path / "three" / "text_index.json"))
    assert tix3 == tix and float(np.abs(np.asarray(merged) - np.asarray(emb)).max()) <= 1e-6
    files = sorted(str(p) for p in (tmp_path / "data").glob("train_*.jsonl"))
    assert write_teacher_scores(files, str(tmp_path / "kd"), emb, tix, R.NumpyDenseIndex(256)) == 5
    with open(tmp_path / "kd" / "train_000.jsonl") as f:
        first = json.loads(f.readline())
    want = float(direct[0] @ direct[1])
    assert abs(first["teacher_pos_score"] - want) <= 2e-6
    second = [json.loads(l) for l in open(tmp_path / "kd" / "train_000.jsonl") if l.strip().startswith("{")][1]
    assert len(second["teacher_neg_scores"]) == 3 and all(s != 0.0 for s in second["teacher_neg_scores"])


def test_cli_encode_arguments(tmp_path):
    from src.train.cli import teacher_scores
    a = teacher_scores.parse_args(["encode", "--model-dir", "m", "--output-dir", "c"])
    assert (a.max_length, a.batch_tokens, a.precision, a.num_shards, a.shard_index, a.merge) == (256, 16384, "bf16", 1, 0, False)
    for bad in (["encode", "--output-dir", "c"], ["encode", "--model-dir", "m", "--output-dir", "c", "--num-shards", "2",
                                                   "--shard-index", "2"],
                ["encode", "--model-dir", "m", "--output-dir", "c", "--precision", "fp16"]):
        with pytest.raises(SystemExit):
            teacher_scores.parse_args(bad)
    with pytest.raises(FileNotFoundError):
        teacher_scores.main(["encode", "--merge", "--output-dir", str(tmp_path)])
