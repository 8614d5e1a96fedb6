"""Host side of the multi-vector search: MultiVectorIndex's argument rules and mine_multivector_negatives over an injected
encoder and a pure-torch index built on maxsim_pairs_torch.  No GPU."""
import json

import pytest
import torch

D = 64


def _rows(n, seed=0):
    x = torch.randn(n, D, generator=torch.Generator().manual_seed(seed))
    return x / x.norm(dim=-1, keepdim=True)


def test_index_argument_errors():
    from snx.retrieval import MultiVectorIndex
    for dim in (0, 96, 2048, 64.0, True):
        with pytest.raises(ValueError):
            MultiVectorIndex(dim, "cpu")
    index = MultiVectorIndex(D, "cpu")
    with pytest.raises(RuntimeError):
        index.search(_rows(2), [0, 2], 1)                          # before build
    for mv, ptr in ((_rows(4).double(), [0, 4]), (_rows(4)[:, :32], [0, 4]), (_rows(4), [1, 4]), (_rows(4), [0, 3, 2]),
                    (_rows(4), [0, 5]), (_rows(4), [0.0, 4.0])):
        with pytest.raises(ValueError):
            index.add(mv, ptr)
    index.add(_rows(5), [0, 2, 2, 5])                              # a document without rows is legal
    with pytest.raises(ValueError):
        index.add(_rows(3).bfloat16(), [0, 3])                     # one dtype per index
    index.build()
    assert index.num_docs == 3 and index.num_rows == 5
    q = _rows(3, 1)
    for bad in (lambda: index.search(q, [0, 3], 0), lambda: index.search(q, [0, 3], 1025),
                lambda: index.search(q.bfloat16(), [0, 3], 1), lambda: index.search(q, [0, 4], 1),
                lambda: index.search(q, [0, 1, 1, 3], 1),          # a query without rows
                lambda: index.search(q, [0, 3], 1, chunk_docs=63), lambda: index.search(q, [0, 3], 1, query_slice=-1),
                lambda: index.search_band(q, [0, 3], 2, 2), lambda: index.search_band(q, [0, 3], 0, 1025)):
        with pytest.raises(ValueError):
            bad()


class _TorchIndex:
    """MultiVectorIndex's methods as the miner uses them, on maxsim_pairs_torch."""

    def __init__(self):
        self.parts, self.ptr, self.calls = [], [0], []

    def add(self, mv, ptr):
        self.parts.append(mv)
        self.ptr += [self.ptr[-1] + int(v) for v in list(ptr)[1:]]

    def build(self):
        self.rows = torch.cat(self.parts)

    def _all(self, qmv, q_ptr):
        from snx.teacher import maxsim_pairs_torch
        nq, nd = len(q_ptr) - 1, len(self.ptr) - 1
        joint = list(q_ptr) + [q_ptr[-1] + v for v in self.ptr[1:]]
        pq = [q for q in range(nq) for _ in range(nd)]
        pd = [nq + d for _ in range(nq) for d in range(nd)]
        return maxsim_pairs_torch(torch.cat([qmv, self.rows]), joint, pq, pd).view(nq, nd)

    def search_band(self, qmv, q_ptr, lo, hi, exclude=None, chunk_docs=0):
        s = self._all(qmv, q_ptr)
        self.calls.append((lo, hi, [list(e) for e in exclude]))
        scores, docs = torch.zeros(len(s), hi - lo), torch.full((len(s), hi - lo), -1, dtype=torch.int32)
        found = torch.zeros(len(s), dtype=torch.int32)
        for q in range(len(s)):
            order = [d for d in sorted(range(s.shape[1]), key=lambda d: (-float(s[q, d]), d)) if d not in exclude[q]][lo:hi]
            found[q] = len(order)
            for j, d in enumerate(order):
                scores[q, j], docs[q, j] = s[q, d], d
        return scores, docs, found

    def pair_scores(self, qmv, q_ptr, pairs):
        s = self._all(qmv, q_ptr)
        return torch.stack([s[int(q), int(d)] for q, d in pairs.tolist()]).float()


def test_mine_multivector_negatives(tmp_path):
    from src.train.mining.multivector import mine_multivector_negatives
    texts = {f"d{i}": _rows(2 + i % 3, 10 + i) for i in range(8)}
    texts.update({"qa": texts["d0"][:1] * 1.0, "qb": _rows(2, 50)})
    recs = [{"query": "qa", "positive": "d0", "source": "s"}, {"query": "qa", "positive": "d1"},
            {"query": "qb", "positive": "d2", "negatives": ["x"]}, {"query": 7, "positive": "d3"}] + \
           [{"query": "qb", "positive": f"d{i}"} for i in range(4, 8)]
    src = tmp_path / "in" / "train_0.jsonl"
    src.parent.mkdir()
    src.write_text("".join(json.dumps(r) + "\n" for r in recs))

    def encode_mv(batch):
        ptr = torch.tensor([0] + [len(texts[t]) for t in batch]).cumsum(0)
        return None, ptr, torch.cat([texts[t] for t in batch])

    index = _TorchIndex()
    out = mine_multivector_negatives([str(src)], str(tmp_path / "out"), encode_mv, index, k=3, rank_start=2, rank_end=4,
                                     chunk_texts=3)
    docs = [f"d{i}" for i in (0, 1, 2, 4, 5, 6, 7)]              # unique positives of the scoreable records, in order
    assert index.ptr == torch.tensor([0] + [len(texts[t]) for t in docs]).cumsum(0).tolist()
    assert [c[:2] for c in index.calls] == [(2, 4)] and index.calls[0][2] == [[0, 1], [2, 3, 4, 5, 6]]
    got = [json.loads(x) for x in (tmp_path / "out" / "train_0.jsonl").read_text().splitlines()]
    assert got[3] == recs[3]                                       # no string query: unchanged
    s = index._all(torch.cat([texts["qa"], texts["qb"]]), [0, 1, 3])
    order = [d for d in sorted(range(7), key=lambda d: (-float(s[0, d]), d)) if d not in (0, 1)][2:4]
    assert got[0] == {"query": "qa", "positive": "d0", "negatives": [docs[d] for d in order] + [docs[order[-1]]],
                      "teacher_pos_score": round(float(s[0, 0]), 6),
                      "teacher_neg_scores": [round(float(s[0, d]), 6) for d in order + order[-1:]], "source": "s"}
    assert got[1]["negatives"] == got[0]["negatives"] and got[1]["teacher_pos_score"] == round(float(s[0, 1]), 6)
    assert got[2] == recs[2] and got[4] == recs[4]                 # qb: two non-positives, none at rank 2
    assert list(got[0]) == ["query", "positive", "negatives", "teacher_pos_score", "teacher_neg_scores", "source"]
    assert (out["records"], out["queries"], out["docs"], out["padded"], out["unchanged"]) == (8, 2, 7, 2, 6)
    assert out["store_rows"] == index.ptr[-1] and out["store_bytes"] == index.ptr[-1] * D * 4
