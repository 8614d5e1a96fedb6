"""Multi-vector teacher scores, the parts that need no GPU: the float64 restatement of MaxSim on a hand-worked example, the
argument rules, the weighted combination, and the record handling of ``teacher_scores score-mv`` over a stub encoder."""
import json

import pytest
import torch

from snx.teacher import maxsim_pairs, maxsim_pairs_torch


def _rows(*vecs, D=64):
    out = torch.zeros(len(vecs), D)
    for i, v in enumerate(vecs):
        out[i, :len(v)] = torch.tensor(v)
    return out


def test_maxsim_pairs_torch_on_a_hand_worked_example():
    # query rows (1, 0) and (0, 1); document rows (0.6, 0.8), (-1, 0), (0.5, -0.5):
    # S = [[0.6, -1, 0.5], [0.8, 0, -0.5]] -> row maxima 0.6 and 0.8 -> mean 0.7
    # the other way round: S^T -> maxima 0.8, 0, 0.5 -> mean 1.3 / 3
    mv = _rows((1.0, 0.0), (0.0, 1.0), (0.6, 0.8), (-1.0, 0.0), (0.5, -0.5))
    got = maxsim_pairs_torch(mv, [0, 2, 5], [0, 1, 0], [1, 0, 0])
    assert got.dtype == torch.float64
    want = torch.tensor([0.7, 1.3 / 3.0, 1.0], dtype=torch.float64)
    assert float((got - want).abs().max()) <= 1e-7                 # the inputs are fp32 numbers (0.6, 0.8)


@pytest.mark.parametrize("scorer", (maxsim_pairs, maxsim_pairs_torch))
def test_argument_rules(scorer):
    mv = _rows((1.0,), (0.5,), (0.25,))
    with pytest.raises(ValueError, match="no multi-vector row"):   # sequence 1 is empty: either side
        scorer(mv, [0, 3, 3], [0], [1])
    with pytest.raises(ValueError, match="no multi-vector row"):
        scorer(mv, [0, 3, 3], [1], [0])
    for bad in (2, -1):
        with pytest.raises(ValueError, match="outside"):
            scorer(mv, [0, 2, 3], [0], [bad])
    with pytest.raises(ValueError, match="multiple of 64"):
        scorer(torch.zeros(3, 96), [0, 2, 3], [0], [1])
    with pytest.raises(ValueError, match="multiple of 64"):
        scorer(torch.zeros(3, 1088), [0, 2, 3], [0], [1])
    with pytest.raises(ValueError, match="mv_ptr"):
        scorer(mv, [0, 2, 4], [0], [1])


def test_weighted_combination():
    from src.model.teachers import combine_scores
    dense, colbert = torch.tensor([0.5, 0.2]), torch.tensor([0.9, 0.4])
    assert torch.allclose(combine_scores(dense, colbert, (1.0, 3.0)), torch.tensor([0.8, 0.35]))
    assert torch.equal(combine_scores(dense, colbert, (0.0, 2.0)), colbert)
    assert torch.equal(combine_scores(dense, colbert, (5.0, 0.0)), dense)
    with pytest.raises(ValueError):
        combine_scores(dense, colbert, (0.0, 0.0))


@pytest.mark.parametrize("mode", ("colbert", "dense+colbert"))
def test_score_mv_record_handling(tmp_path, mode):
    from src.train.mining.multivector import write_multivector_scores
    gen = torch.Generator().manual_seed(5)
    vectors, calls = {}, []

    def encode_mv(texts):
        """A stub encoder: per text a fixed set of len(words) + 1 unit rows and a fixed unit embedding."""
        calls.append(list(texts))
        for t in texts:
            if t not in vectors:
                v = torch.randn(len(t.split()) + 2, 64, generator=gen)
                vectors[t] = v / v.norm(dim=-1, keepdim=True)
        ptr = [0]
        for t in texts:
            ptr.append(ptr[-1] + vectors[t].shape[0] - 1)
        return (torch.stack([vectors[t][0] for t in texts]), torch.tensor(ptr), torch.cat([vectors[t][1:] for t in texts]))

    records = [{"query": "q one", "positive": "p one", "negative": "n one", "id": 7},
               {"query": "q one", "positive": "p two", "negatives": ["n one", "n two words", None]},
               {"query": "q two", "positive": None},
               {"query": "q three", "positive": "p one"}]
    src = tmp_path / "in" / "train_0.jsonl"
    src.parent.mkdir()
    src.write_text("".join(json.dumps(r) + "\n" for r in records))
    n = write_multivector_scores([str(src)], str(tmp_path / "out"), encode_mv, maxsim_pairs_torch, mode=mode,
                                 weights=(1.0, 2.0), chunk_records=3)
    out = [json.loads(l) for l in (tmp_path / "out" / "train_0.jsonl").read_text().splitlines()]
    assert n == 3 and len(out) == 4 and len(calls) == 2            # two chunks, each encoded once
    assert sorted(calls[0]) == sorted({"q one", "p one", "n one", "p two", "n two words"})      # every text once

    def want(q, d):
        mv = torch.cat([vectors[q][1:], vectors[d][1:]])
        nq = vectors[q].shape[0] - 1
        colbert = float(maxsim_pairs_torch(mv, [0, nq, mv.shape[0]], [0], [1])[0].to(torch.float32))
        if mode == "colbert":
            return round(colbert, 6)                               # exactly the field: the score as fp32, six decimals
        dense = float((vectors[q][0] * vectors[d][0]).sum())
        return pytest.approx(round((dense + 2.0 * colbert) / 3.0, 6), abs=2e-6)

    assert out[0]["teacher_pos_score"] == want("q one", "p one")
    assert out[0]["teacher_neg_score"] == want("q one", "n one")
    assert out[0]["id"] == 7 and "teacher_neg_scores" not in out[0]
    assert out[1]["teacher_neg_score"] == 0.0                      # no `negative`: 0.0, as `score` writes it
    assert out[1]["teacher_neg_scores"][:2] == [want("q one", "n one"), want("q one", "n two words")]
    assert out[1]["teacher_neg_scores"][2] == 0.0
    assert out[2] == records[2]                                    # no positive: written unchanged
    assert out[3]["teacher_pos_score"] == want("q three", "p one")
