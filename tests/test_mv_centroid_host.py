"""Host side of the multi-vector candidate search: the argument rules of MultiVectorIndex's centroid methods and
mine_multivector_negatives(index_type="centroid") over an injected encoder and a stub index.  No GPU."""
import json

import pytest
import torch

D = 64


def _rows(n, seed=0):
    x = torch.randn(n, D, generator=torch.Generator().manual_seed(seed))
    return x / x.norm(dim=-1, keepdim=True)


def test_centroid_argument_errors():
    from snx.retrieval import MultiVectorIndex
    index = MultiVectorIndex(D, "cpu")
    index.add(_rows(5), [0, 2, 2, 5])
    with pytest.raises(RuntimeError):
        index.train_centroids(4)                                   # before build
    index.build()
    for nc in (0, 4097, 2.0, True):
        with pytest.raises(ValueError):
            index.train_centroids(nc)
    for c in (_rows(4)[:, :32], _rows(4).double(), _rows(4)[0], torch.zeros(0, D), torch.zeros(4097, D),
              _rows(4).to("meta")):                                # wrong shape / dtype / count / device
        with pytest.raises(ValueError):
            index.set_centroids(c)
    q = _rows(3, 1)
    with pytest.raises(RuntimeError):
        index.candidates(q, [0, 3], 2)                             # before centroids exist
    with pytest.raises(RuntimeError):
        index.search_two_phase(q, [0, 3], 1, 2)
    index.centroids, index.codes = _rows(2), torch.zeros(5, dtype=torch.uint16)   # as an assignment leaves them
    for bad in (lambda: index.candidates(q, [0, 3], 0), lambda: index.candidates(q, [0, 3], 1025),
                lambda: index.candidates(q, [0, 3], 2.0), lambda: index.search_two_phase(q, [0, 3], 3, 2),
                lambda: index.search_band_two_phase(q, [0, 3], 0, 3, 2),             # hi > ncand
                lambda: index.search_band_two_phase(q, [0, 3], 2, 2, 8),
                lambda: index.candidates(q, [0, 3], 2, chunk_docs=63)):
        with pytest.raises(ValueError):
            bad()
    index.add(_rows(2), [0, 2])                                    # a later add invalidates both
    assert index.centroids is None and index.codes is None and not index.built


class _StubIndex:
    """The index as the miner uses it: the band is the documents in id order, a score is -(doc id)."""

    def __init__(self):
        self.nd, self.calls = 0, []

    def add(self, mv, ptr):
        self.nd += len(ptr) - 1

    def build(self):
        pass

    def train_centroids(self, ncentroids):
        self.calls.append(("train", ncentroids))

    def _band(self, nq, lo, hi, exclude):
        scores, docs = torch.zeros(nq, hi - lo), torch.full((nq, hi - lo), -1, dtype=torch.int32)
        found = torch.zeros(nq, dtype=torch.int32)
        for q in range(nq):
            order = [d for d in range(self.nd) if d not in exclude[q]][lo:hi]
            found[q] = len(order)
            for j, d in enumerate(order):
                scores[q, j], docs[q, j] = -float(d), d
        return scores, docs, found

    def search_band(self, qmv, q_ptr, lo, hi, exclude=None, chunk_docs=0):
        self.calls.append(("exact", lo, hi))
        return self._band(len(q_ptr) - 1, lo, hi, exclude)

    def search_band_two_phase(self, qmv, q_ptr, lo, hi, ncand, exclude=None, chunk_docs=0):
        self.calls.append(("centroid", lo, hi, ncand))
        return self._band(len(q_ptr) - 1, lo, hi, exclude)

    def pair_scores(self, qmv, q_ptr, pairs):
        return torch.tensor([-float(d) for _, d in pairs.tolist()])


def test_mine_centroid_writes_the_exact_layout(tmp_path):
    from src.train.mining.multivector import default_ncand, mine_multivector_negatives
    texts = {f"d{i}": _rows(2, 10 + i) for i in range(6)}
    texts.update({"qa": _rows(1, 40), "qb": _rows(2, 50)})
    recs = [{"query": "qa", "positive": "d0", "source": "s"}, {"query": "qb", "positive": "d1"}] + \
           [{"query": "qb", "positive": f"d{i}"} for i in range(2, 6)]
    src = tmp_path / "in" / "train_0.jsonl"
    src.parent.mkdir()
    src.write_text("".join(json.dumps(r) + "\n" for r in recs))

    def encode_mv(batch):
        ptr = torch.tensor([0] + [len(texts[t]) for t in batch]).cumsum(0)
        return None, ptr, torch.cat([texts[t] for t in batch])

    outs, stubs = {}, {}
    for kind in ("exact", "centroid"):
        stubs[kind] = _StubIndex()
        counts = mine_multivector_negatives([str(src)], str(tmp_path / kind), encode_mv, stubs[kind], k=2, rank_start=1,
                                            rank_end=3, index_type=kind, ncentroids=16)
        outs[kind] = (counts, (tmp_path / kind / "train_0.jsonl").read_text())
    assert outs["exact"] == outs["centroid"]
    assert stubs["exact"].calls == [("exact", 1, 3)]
    assert stubs["centroid"].calls == [("train", 16), ("centroid", 1, 3, default_ncand(3))] and default_ncand(3) == 128
    assert (default_ncand(50), default_ncand(1000)) == (200, 1024)
    with pytest.raises(ValueError):
        mine_multivector_negatives([str(src)], str(tmp_path / "x"), encode_mv, _StubIndex(), index_type="ivf")
    with pytest.raises(ValueError):
        mine_multivector_negatives([str(src)], str(tmp_path / "x"), encode_mv, _StubIndex(), rank_end=50,
                                   index_type="centroid", ncand=20)
