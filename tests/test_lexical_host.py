"""Lexical teacher scores, the parts that need no GPU: the torch restatements against dict loops, the sparse head's file, the
argument rules, ``combine_modes``, and the new modes of ``get_ranking_scores`` / ``score-mv`` over a CPU encoder."""
import dataclasses
import json

import pytest
import torch

from snx.teacher import (TeacherEncoder, lexical_pairs, lexical_pairs_torch, lexical_weights_torch, maxsim_pairs_torch,
                         random_colbert_head, random_sparse_head)
from src.model.teachers import BGEM3Teacher, combine_modes
from tests import teacher_helpers as TH


class Tok(TH.ToyTokenizer):
    cls_token_id, eos_token_id, pad_token_id = 0, 2, 1             # what encode_m3 leaves out by default


def test_torch_restatements_agree_with_dict_loops():
    gen = torch.Generator().manual_seed(3)
    ids = torch.randint(0, 12, (5, 40), generator=gen)
    mask = (torch.arange(40)[None, :] < torch.tensor([40, 1, 17, 33, 2])[:, None]).long()
    tw = torch.relu(torch.randn(5, 40, generator=gen, dtype=torch.float64))
    ids[1, 0] = 7                                                  # a sequence of one unused id: no term
    want = []
    for row, m, t in zip(ids.tolist(), mask.tolist(), tw.tolist()):
        want.append({})
        for v, keep, x in zip(row, m, t):
            if keep and v not in (0, 7) and x > 0:
                want[-1][v] = max(want[-1].get(v, 0.0), x)
    ptr, li, lw = lexical_weights_torch(ids, mask, tw, [0, 7])
    got = [dict(zip(li[a:b].tolist(), lw[a:b].tolist())) for a, b in zip(ptr.tolist(), ptr.tolist()[1:])]
    assert got == want and got[1] == {} and all(li[a:b].tolist() == sorted(d) for a, b, d in zip(ptr, ptr[1:], want))
    pq, pd = [0, 0, 1, 2, 3, 4], [3, 0, 2, 1, 4, 2]
    ref = [sum(x * want[b][v] for v, x in want[a].items() if v in want[b]) for a, b in zip(pq, pd)]
    assert torch.allclose(lexical_pairs_torch(ptr, li, lw, pq, pd), torch.tensor(ref, dtype=torch.float64), rtol=1e-14, atol=0)
    for scorer in (lexical_pairs, lexical_pairs_torch):           # the argument rules, before any device is asked for
        for bad in (5, -1):
            with pytest.raises(ValueError, match="outside"):
                scorer(ptr, li, lw.float(), [0], [bad])
        with pytest.raises(ValueError, match="lex_ptr"):
            scorer(ptr + 1, li, lw.float(), [0], [1])
    with pytest.raises(ValueError, match="at most 8"):
        lexical_weights_torch(ids, mask, tw, list(range(9)))


@pytest.fixture
def model_dir(tmp_path):
    _, cfg, sd = TH.golden()
    (tmp_path / "config.json").write_text(json.dumps({"model_type": "xlm-roberta", **dataclasses.asdict(cfg)}))
    torch.save(sd, tmp_path / "pytorch_model.bin")
    torch.save(random_colbert_head(cfg, 77), tmp_path / "colbert_linear.pt")
    torch.save(random_sparse_head(cfg, 79), tmp_path / "sparse_linear.pt")
    return tmp_path


def _score_mv(model_dir, src, *more):
    from src.train.cli import teacher_scores
    return teacher_scores.main(["score-mv", "--model-dir", str(model_dir), "--input-pattern", str(src), "--val-pattern",
                                str(model_dir / "none"), "--output-dir", str(model_dir / "out"), "--precision", "fp32",
                                "--device", "cpu", "--max-length", "64", *more], tokenizer=Tok())


def test_the_sparse_head_file_and_a_missing_head(model_dir):
    _, cfg, sd = TH.golden()
    enc = TeacherEncoder.from_pretrained(str(model_dir), device="cpu", precision="fp32")
    assert enc.has_sparse and torch.equal(enc.sparse["weight"], random_sparse_head(cfg, 79)["weight"])
    with pytest.raises(ValueError, match="at most 8"):
        enc.encode_tokens_m3(*TH.pad_batch(TH.ragged_sequences([5, 9])), list(range(9)))
    with pytest.raises(ValueError, match="8192"):                  # refused before any forward
        enc.encode_tokens_m3(torch.zeros(1, 8193, dtype=torch.long), torch.ones(1, 8193, dtype=torch.long), [])
    torch.save({"weight": torch.zeros(cfg.hidden_size), "bias": torch.zeros(1)}, model_dir / "sparse_linear.pt")
    with pytest.raises(ValueError, match="sparse head"):           # weight [H] instead of [1, H]
        TeacherEncoder.from_pretrained(str(model_dir), device="cpu")
    (model_dir / "sparse_linear.pt").unlink()
    (model_dir / "train_0.jsonl").write_text(json.dumps({"query": "a", "positive": "b"}) + "\n")
    with pytest.raises(FileNotFoundError, match="sparse_linear.pt"):
        _score_mv(model_dir, model_dir / "train_0.jsonl", "--mode", "sparse")
    teacher = BGEM3Teacher(TeacherEncoder.from_pretrained(str(model_dir), device="cpu"), device="cpu", tokenizer=Tok())
    with pytest.raises(ValueError, match="sparse_linear.pt"):
        teacher.get_ranking_scores(["a"], ["b"], mode="dense+sparse")
    only = TeacherEncoder(cfg, sd, "cpu", "fp32", sparse_head=random_sparse_head(cfg, 79))
    with pytest.raises(ValueError, match="colbert_linear.pt"):
        BGEM3Teacher(only, device="cpu", tokenizer=Tok()).get_ranking_scores(["a"], ["b"], mode="sparse+colbert")


def test_combine_modes():
    s = {"dense": torch.tensor([0.5, 0.2]), "sparse": torch.tensor([2.0, 0.0]), "colbert": torch.tensor([0.9, 0.4])}
    w = {"dense": 1.0, "sparse": 2.0, "colbert": 3.0}
    assert torch.allclose(combine_modes(s, w), torch.tensor([(0.5 + 4.0 + 2.7) / 6.0, (0.2 + 1.2) / 6.0]))
    assert all(torch.equal(x, s["sparse"]) for x in (combine_modes({"sparse": s["sparse"]}, w),
                                                     combine_modes(s, {"dense": 0.0, "sparse": 5.0, "colbert": 0.0})))
    for bad in ({"dense": 0.0, "sparse": 0.0, "colbert": 0.0}, {"dense": -1.0, "sparse": 1.0, "colbert": 1.0}, {"dense": 1.0}):
        with pytest.raises(ValueError):
            combine_modes(s, bad)


@pytest.mark.parametrize("mode", ("sparse", "dense+sparse", "sparse+colbert", "dense+sparse+colbert"))
def test_new_modes_of_ranking_scores_and_score_mv(model_dir, mode):
    enc = TeacherEncoder.from_pretrained(str(model_dir), device="cpu", precision="fp32")
    teacher = BGEM3Teacher(enc, device="cpu", tokenizer=Tok(), max_length=64)
    q, d = ["what is a cat", "rain in spain", "dogs bark"], ["a cat is a small animal that purrs", "rain in spain", "x"]
    w, got = {"dense": 1.0, "sparse": 2.0, "colbert": 0.5}, teacher.get_ranking_scores(q, d, mode=mode, weights=(1.0, 2.0, 0.5))
    emb, mv_ptr, mv, lex_ptr, li, lw = teacher.encode_m3(q + d)
    lex = teacher.compute_lexical_scores(q, [[t] for t in d])
    assert float(lex[1]) > 0 and float(lex[2]) == 0.0              # the same text twice; no word in common
    parts = {"dense": (emb[:3] * emb[3:]).sum(-1), "sparse": torch.cat(lex),
             "colbert": maxsim_pairs_torch(mv, mv_ptr, [0, 1, 2], [3, 4, 5]).float()}
    want = sum(w[m] * parts[m] for m in mode.split("+")) / sum(w[m] for m in mode.split("+"))
    assert torch.allclose(got, want, rtol=1e-6, atol=1e-7)
    src = model_dir / "train_0.jsonl"                              # score-mv: the record handling of test_maxsim_host.py
    src.write_text(json.dumps({"query": q[0], "positive": d[0], "negatives": [d[2], None], "id": 7}) + "\n" +
                   json.dumps({"query": q[1], "positive": None}) + "\n" + json.dumps({"query": q[1], "positive": d[1]}) + "\n")
    assert _score_mv(model_dir, src, "--mode", mode, "--sparse-weight", "2", "--colbert-weight", "0.5") == 2
    out = [json.loads(l) for l in (model_dir / "out" / "train_0.jsonl").read_text().splitlines()]
    assert out[0]["teacher_pos_score"] == pytest.approx(float(want[0]), abs=2e-6) and out[0]["id"] == 7
    assert out[0]["teacher_neg_scores"][1] == 0.0 and out[0]["teacher_neg_score"] == 0.0
    assert out[1] == {"query": q[1], "positive": None}
    assert out[2]["teacher_pos_score"] == pytest.approx(float(want[1]), abs=2e-6)
